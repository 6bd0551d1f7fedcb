// mot_lincore.hip -- the kernels the linear front-ends share (mot_lincore.hpp), each with its launcher: rows_finish_kernel, the
// forward's last pass; rows_norm_bwd_kernel, the way back through its norm; count_pads_kernel, the id statistics.  The two row
// kernels give one wave a row and lane l the 16-byte chunks l, l + 64, ... of it, the whole row (<= kRowMaxDim columns) in
// registers between the reduction and the store; a lane adds chunk by chunk and element by element into ONE fp32, so every caller
// sums in the same order.  `vec` (from the launcher) says that dim, strides and pointers allow the chunks; else a lane walks
// elements l, l + 64, ... and reads the row twice.
#include "mot_lincore.hpp"
#include "mot_mix.hpp"

namespace mot {

// y <- r s, s = y (+ the token row), r = rsqrt(mean(s^2) + eps) or 1.  bf16: y arrives rounded by the product kernel, s = tok + y is
// rounded before the squares are taken and r s on store -- the roundings of the reference's bf16 runs (F.linear, the add, rms_norm's
// result; train_gpt.py:172-173, 185-186).
template <typename T, bool kTok>
__global__ __launch_bounds__(kThreads) void rows_finish_kernel(T *__restrict__ y, const int32_t *__restrict__ tokens, const T *__restrict__ tok_table,
                                                               int64_t tok_rows, int64_t n, int dim, int norm, int vec, float eps,
                                                               float *__restrict__ row_rnorm, uint32_t *status) {
    using vec_t = typename Elem<T>::vec;
    constexpr int VEC = Elem<T>::kVec, NCH = kRowMaxDim / VEC / 64;   // chunks a lane holds: 8 of 4 floats, 4 of 8 bf16
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= n) return;
    T *p = y + r * dim;
    const T *trow = nullptr;
    if constexpr (kTok) {
        int tok = __builtin_amdgcn_readfirstlane(tokens[r]);   // wave-uniform: the token row's base stays in scalar registers
        if ((uint64_t)(uint32_t)tok >= (uint64_t)tok_rows) {
            if (status && lane == 0) atomicOr(status, kStatusTokenOor);
            tok = 0;
        }
        trow = tok_table + (int64_t)tok * dim;
    }
    float ss = 0.f, rs = 1.0f;
    if (vec) {
        const int nv = dim / VEC;
        vec_t s[NCH];   // a chunk past the row's end is 0 and adds 0: the loads are the only code under the test, which keeps the chunks in
#pragma unroll          // registers of their own (with the sums under it too the compiler carries all of them as one 32-register value)
        for (int i = 0; i < NCH; ++i) {
            const int j = lane + 64 * i;
            if constexpr (kTok) s[i] = j < nv ? Elem<T>::loadv(p + VEC * j) + Elem<T>::loadv(trow + VEC * j) : (vec_t)(0.f);
            else s[i] = j < nv ? Elem<T>::loadv(p + VEC * j) : (vec_t)(0.f);
            if constexpr (kTok && sizeof(T) == 2) s[i] = __builtin_convertvector(__builtin_convertvector(s[i], bf16x8v), float8v);   // s = bf16(tok + y)
#pragma unroll
            for (int e = 0; e < VEC; ++e) ss += s[i][e] * s[i][e];
        }
        if (norm) rs = rms_scale(wave_sum(ss), dim, eps);
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int j = lane + 64 * i;
            if (j < nv) Elem<T>::storev_nt(p + VEC * j, s[i] * rs);
        }
    } else {
        auto s_at = [&](int j) {
            float v = (float)p[j];
            if constexpr (kTok) v = (float)(T)(v + (float)trow[j]);
            return v;
        };
        for (int j = lane; j < dim; j += 64) { const float v = s_at(j); ss += v * v; }
        if (norm) rs = rms_scale(wave_sum(ss), dim, eps);
        for (int j = lane; j < dim; j += 64) p[j] = (T)(s_at(j) * rs);
    }
    if (row_rnorm && lane == 0) row_rnorm[r] = rs;
}

// dy = r (g - x mean(g x)), or g; to dy in T (the operand of the bf16 products) and / or to dy32 in fp32
template <typename T>
__global__ __launch_bounds__(kThreads) void rows_norm_bwd_kernel(const T *__restrict__ g, const T *__restrict__ x, const float *__restrict__ rnorm, int64_t n,
                                                                 int dim, int norm, int vec, T *__restrict__ dy, int64_t ld, float *__restrict__ dy32,
                                                                 int64_t ld32) {
    using vec_t = typename Elem<T>::vec;
    constexpr int VEC = Elem<T>::kVec, NCH = kRowMaxDim / VEC / 64;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= n) return;
    const T *gr = g + r * dim, *xr = x + r * dim;
    T *dr = dy + r * ld;
    float *dr32 = dy32 + r * ld32;
    float m = 0.f, ry = 1.0f;
    if (vec) {
        const int nv = dim / VEC;
        vec_t gv[NCH], xv[NCH];   // past the row's end 0, as above
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int j = lane + 64 * i;
            gv[i] = j < nv ? Elem<T>::loadv(gr + VEC * j) : (vec_t)(0.f);
            xv[i] = j < nv && norm ? Elem<T>::loadv(xr + VEC * j) : (vec_t)(0.f);
#pragma unroll
            for (int e = 0; e < VEC; ++e) m += gv[i][e] * xv[i][e];
        }
        if (norm) {
            m = wave_sum(m) / (float)dim;
            ry = rnorm[r];
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int j = lane + 64 * i;
            if (j < nv) {
                const vec_t d = norm ? (gv[i] - xv[i] * m) * ry : gv[i];
                if (dy) Elem<T>::storev_nt(dr + VEC * j, d);
                if (dy32) {
#pragma unroll
                    for (int q = 0; q < VEC / 4; ++q) *(float4v *)(dr32 + VEC * j + 4 * q) = float4v{d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
                }
            }
        }
        return;
    }
    if (norm) {
        for (int j = lane; j < dim; j += 64) m += (float)gr[j] * (float)xr[j];
        m = wave_sum(m) / (float)dim;
        ry = rnorm[r];
    }
    for (int j = lane; j < dim; j += 64) {
        const float d = norm ? ((float)gr[j] - (float)xr[j] * m) * ry : (float)gr[j];
        if (dy) dr[j] = (T)d;
        if (dy32) dr32[j] = d;
    }
}

// the statistics of runs/79_*.py:484-488 from the two id tensors as the fused front-end counts them: tokens, byte slots and, with
// ids from the token->byte table, pads before and after the pull (padded == nullptr: ids given, the first two only)
__global__ __launch_bounds__(kThreads) void count_pads_kernel(const int64_t *__restrict__ padded, const int64_t *__restrict__ after, int64_t n_slots,
                                                              int64_t pad, int64_t n_tokens, int64_t *counters) {
    if (padded) {
        int before = 0, aft = 0;
        for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n_slots; i += (int64_t)gridDim.x * kThreads) {
            before += padded[i] == pad;
            aft += after[i] == pad;
        }
        before = (int)wave_sum((float)before);   // <= 64 * a few thousand per wave: exact in fp32
        aft = (int)wave_sum((float)aft);
        if ((threadIdx.x & 63) == 0) {
            atomicAdd((unsigned long long *)counters + 2, (unsigned long long)before);
            atomicAdd((unsigned long long *)counters + 3, (unsigned long long)aft);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd((unsigned long long *)counters + 0, (unsigned long long)n_tokens);
        atomicAdd((unsigned long long *)counters + 1, (unsigned long long)n_slots);
    }
}

// ------------------------------------------------------------------------------------------ launchers
static unsigned row_blocks(int64_t n) { return (unsigned)((n + kWaves - 1) / kWaves); }
// the 16-byte chunks apply: whole chunks per row and per stride, every base on a 16-byte address
static int rows_vec(int dim, int elem_bytes, uintptr_t bases, int64_t stride_bytes) {
    return dim <= kRowMaxDim && (((size_t)dim * elem_bytes | (size_t)stride_bytes | bases) & 15) == 0;
}

template <typename T, bool kTok>
static int rows_finish(void *y, const int32_t *tokens, const void *tok_table, int64_t tok_rows, int64_t n, int dim, int norm, float eps, float *row_rnorm,
                       uint32_t *status, hipStream_t stream) {
    if (n <= 0) return MOT_OK;
    const int vec = rows_vec(dim, sizeof(T), (uintptr_t)y | (uintptr_t)tok_table, 0);
    hipLaunchKernelGGL((rows_finish_kernel<T, kTok>), dim3(row_blocks(n)), dim3(kThreads), 0, stream, (T *)y, tokens, (const T *)tok_table, tok_rows, n, dim,
                       norm, vec, eps, row_rnorm, status);
    return check_launch("rows_finish_kernel");
}

int launch_rows_finish(void *y, int64_t n, int dim, int norm, float eps, float *row_rnorm, int dtype, hipStream_t stream) {
    return dtype == MOT_BF16 ? rows_finish<__bf16, false>(y, nullptr, nullptr, 0, n, dim, norm, eps, row_rnorm, nullptr, stream)
                             : rows_finish<float, false>(y, nullptr, nullptr, 0, n, dim, norm, eps, row_rnorm, nullptr, stream);
}
int launch_rows_finish_tok(void *y, const int32_t *tokens, const void *tok_table, int64_t tok_rows, int64_t n, int dim, int norm, float eps,
                           float *row_rnorm, uint32_t *status, int dtype, hipStream_t stream) {
    return dtype == MOT_BF16 ? rows_finish<__bf16, true>(y, tokens, tok_table, tok_rows, n, dim, norm, eps, row_rnorm, status, stream)
                             : rows_finish<float, true>(y, tokens, tok_table, tok_rows, n, dim, norm, eps, row_rnorm, status, stream);
}

template <typename T>
static int rows_norm_bwd(const void *g, const void *x, const float *rnorm, int64_t n, int dim, int norm, void *dy, int64_t ld, float *dy32, int64_t ld32,
                         hipStream_t stream) {
    if (n <= 0) return MOT_OK;
    const int vec = rows_vec(dim, sizeof(T), (uintptr_t)g | (uintptr_t)x | (uintptr_t)dy | (uintptr_t)dy32,
                             (dy ? ld * (int64_t)sizeof(T) : 0) | (dy32 ? ld32 * 4 : 0));
    hipLaunchKernelGGL(rows_norm_bwd_kernel<T>, dim3(row_blocks(n)), dim3(kThreads), 0, stream, (const T *)g, (const T *)x, rnorm, n, dim, norm, vec, (T *)dy,
                       ld, dy32, ld32);
    return check_launch("rows_norm_bwd_kernel");
}

int launch_rows_norm_bwd(const void *g, const void *x, const float *rnorm, int64_t n, int dim, int norm, void *dy, int64_t ld, float *dy32, int64_t ld32,
                         int dtype, hipStream_t stream) {
    return dtype == MOT_BF16 ? rows_norm_bwd<__bf16>(g, x, rnorm, n, dim, norm, dy, ld, dy32, ld32, stream)
                             : rows_norm_bwd<float>(g, x, rnorm, n, dim, norm, dy, ld, dy32, ld32, stream);
}

int launch_count_pads(const int64_t *padded, const int64_t *after, int64_t n_slots, int64_t pad, int64_t n_tokens, int64_t *counters, hipStream_t stream) {
    // 16 slots per thread up to 1024 workgroups; one workgroup when only the two totals are added
    int64_t blocks = padded ? (n_slots + kThreads * 16 - 1) / (kThreads * 16) : 1;
    blocks = blocks > 1024 ? 1024 : blocks < 1 ? 1 : blocks;
    hipLaunchKernelGGL(count_pads_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, padded, after, n_slots, pad, n_tokens, counters);
    return check_launch("count_pads_kernel");
}

}  // namespace mot
