// mot_gemm_f32.hip -- the fp32 matrix products on v_mfma_f32_32x32x2f32 that the backward passes share:
//   launch_gemm_tn            C[j][k] += sum_n A[n][j] B[n][k]   contraction over the rows (weight gradients), atomic accumulate
//   launch_gemm_rows          C[n][c]  = sum_r A[n][r] B[.][.]   row products, B in either layout, optional bias / accumulate
//   launch_gemm_rows_sliced   the same for few rows over a long reduction, cut into slices summed in a fixed order
//   launch_transpose_f32      a k-major weight as the row-major operand of the LDS-DMA kernel (mot_gemm_bf16.hip)
// Callers: the CONCAT_LINEAR and MEAN backward (mot_bwd_linear.hip, mot_bwd_mean.hip), cross-attention (mot_attn.hip), the
// character mixer (mot_swa.hip), byte self-attention (mot_bsa.hip), the byte head (mot_head.hip) and the composed forward
// (mot_linear.hip); the float64 parity tests of the suite call each launcher directly, route by route.
#include "mot_mix.hpp"

namespace mot {

// C[j][k] += sum_n A[n][j] * B[n][k]   (A: n x M, B: n x Nc, C: M x Nc with leading dimension ldc), fp32 MFMA.
// Workgroup = 128 x 128 output block (4 waves as 2 x 2, each 64 x 64 = 2 x 2 tiles of 32 x 32) over one
// slice of the rows; 16 rows per step, double-buffered LDS, rows ARE the MFMA k index so both operands are
// staged in their natural row-major layout.  Partial blocks are accumulated with float atomics
// (128-byte contiguous segments per instruction).
typedef float f32x16b __attribute__((ext_vector_type(16)));
__global__ __launch_bounds__(kThreads) void gemm_tn_kernel(const float *__restrict__ A_, int lda, int M, const float *__restrict__ B_, int ldb,
                                                           int Nc, int64_t n, int64_t rows_per_split, float *__restrict__ C, int ldc) {
    __shared__ __attribute__((aligned(16))) float lA[2][16 * 128], lB[2][16 * 128];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, li = lane & 31;
    const int j0 = blockIdx.x * 128, k0 = blockIdx.y * 128;
    const int64_t r0 = (int64_t)blockIdx.z * rows_per_split, r1 = min(n, r0 + rows_per_split);
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    f32x16b acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    // staging role: 16 rows x 32 float4 per operand = 512 float4 -> 2 per thread
    float4v ra[2], rb[2];
    const bool va = (lda & 3) == 0 && ((uintptr_t)A_ & 15) == 0, vb = (ldb & 3) == 0 && ((uintptr_t)B_ & 15) == 0;   // 16-byte loads allowed
    auto load_stage = [&](int64_t r) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int q = p * kThreads + tid, row = q >> 5, c4 = (q & 31) * 4;
            const int64_t rr = r + row;
            ra[p] = (float4v)(0.f); rb[p] = (float4v)(0.f);
            if (rr < r1) {
                const float *pa = A_ + rr * lda + j0 + c4, *pb = B_ + rr * ldb + k0 + c4;
                if (va && j0 + c4 + 3 < M) ra[p] = *(const float4v *)pa;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e)   // element-wise guards keep ragged right edges correct
                        if (j0 + c4 + e < M) ra[p][e] = pa[e];
                if (vb && k0 + c4 + 3 < Nc) rb[p] = *(const float4v *)pb;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k0 + c4 + e < Nc) rb[p][e] = pb[e];
            }
        }
    };
    auto store_stage = [&](int buf) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int q = p * kThreads + tid;
            *(float4v *)(&lA[buf][q * 4]) = ra[p];
            *(float4v *)(&lB[buf][q * 4]) = rb[p];
        }
    };
    load_stage(r0);
    store_stage(0);
    __syncthreads();
    int buf = 0;
    for (int64_t r = r0; r < r1; r += 16, buf ^= 1) {
        const bool more = r + 16 < r1;
        if (more) load_stage(r + 16);
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
            const float a0 = lA[buf][(kk + h) * 128 + wm + li], a1 = lA[buf][(kk + h) * 128 + wm + 32 + li];
            const float b0 = lB[buf][(kk + h) * 128 + wn + li], b1 = lB[buf][(kk + h) * 128 + wn + 32 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) store_stage(buf ^ 1);
        __syncthreads();
    }
    // C/D layout: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5); A is the "row" (j) operand
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + wm + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, k = k0 + wn + b * 32 + li;
                if (j < M && k < Nc) atomicAdd(C + (int64_t)j * ldc + k, acc[a][b][r]);
            }
}

int launch_gemm_tn(const float *A_, int lda, int M, const float *B_, int ldb, int Nc, int64_t n, float *C, int ldc, hipStream_t stream) {
    if (M <= 0 || Nc <= 0 || n <= 0) return MOT_OK;
    const int gx = (M + 127) / 128, gy = (Nc + 127) / 128;
    int64_t splits = (1024 + gx * gy - 1) / (gx * gy);                  // ~1024 workgroups in total
    int64_t rows_per = ((n + splits - 1) / splits + 15) / 16 * 16;     // whole 16-row steps
    if (rows_per < 256) rows_per = 256;
    splits = (n + rows_per - 1) / rows_per;
    hipLaunchKernelGGL(gemm_tn_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)splits), dim3(kThreads), 0, stream, A_, lda, M, B_, ldb,
                       Nc, n, rows_per, C, ldc);
    return check_launch("gemm_tn_kernel");
}

// C[n][c] = sum_r A[n][r] * (BT ? B[c][r] : B[r][c])   (A: n x R rows, C: n x Nc; leading dimensions lda / ldb / ldc), fp32 MFMA.
// Same block shape and inner loop as gemm_tn_kernel -- 128 x 128 output block, 16 reduction indices per step, both operands in
// LDS as [reduction index][block row / column], one conflict-free ds_read_b32 per MFMA operand -- with the operand whose rows
// are contiguous along r (A always, B when BT) transposed on its way into LDS: a lane takes 4 consecutive r of one row, 4
// lanes one 64-byte row segment, and writes them as four ds_write_b32 down a padded column.  The reduction is whole
// inside the workgroup (plain stores).  The fused gather + norm kernel (mot_linear.hip) runs its dense-row mode at 48 % of
// the fp32 MFMA peak; this loop reaches ~75 %.
template <bool BT>
__device__ __forceinline__ void gemm_rows_body(const float *__restrict__ A_, int lda, int64_t n, const float *__restrict__ B_, int ldb,
                                               int R, int Nc, float *__restrict__ C, int ldc, const float *__restrict__ bias, int accumulate,
                                               bool plain_order = false) {
    // transposed operands sit in LDS with a row stride of 132 floats: the 4 lanes that share a source row (coalesced 64-byte
    // reads) then write to banks 16 apart, two lanes per bank -- the minimum for 64 dword writes
    constexpr int LDA = 132, LDB = BT ? 132 : 128;
    __shared__ __attribute__((aligned(16))) float lA[2][16 * LDA], lB[2][16 * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, li = lane & 31;
    // XCD-aware block order (1-D grid, workgroup ids round-robin over the 8 XCDs): an XCD walks all column blocks of a row panel
    // back to back, so the panel of A is fetched into that XCD's L2 once instead of once per column block
    const int64_t gx = (n + 127) / 128;
    const int gy = (Nc + 127) / 128;
    // (plain_order: gx * gy blocks, no padding -- the sliced few-row launches, where the padded panels were most of the workgroups and
    //  their dispatch most of the time: 132 rows = 2 panels padded to 8, 2816 workgroups of which 704 work, 100 us)
    const int64_t bid = blockIdx.x, seq = plain_order ? bid : bid >> 3, panel = plain_order ? bid / gy : (seq / gy) * 8 + (bid & 7);
    if (panel >= gx) return;   // the grid is padded to whole groups of 8 panels
    const int64_t j0 = panel * 128;
    const int k0 = (int)(seq % gy) * 128;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    // acc is the MFMA accumulator of kFold reduction steps at a time; it is then folded into `sum` with vector adds and
    // restarted, so no fp32 summation chain is longer than 8 * kFold MFMA steps (blocked summation, like the reference's
    // CPU sgemm: one chain over K = 768 ends up 4x as far from the float64 result as the reference, the parity bar is 2x)
    constexpr int kFold = 8;
    f32x16b acc[2][2], sum[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[a][b][r] = 0.f; sum[a][b][r] = 0.f; }
    const bool va = (lda & 3) == 0 && ((uintptr_t)A_ & 15) == 0, vb = (ldb & 3) == 0 && ((uintptr_t)B_ & 15) == 0;
    float4v ra[2], rb[2];
    // rows-contiguous-along-r operand: thread -> (row = q >> 2, 4 consecutive r starting at (q & 3) * 4): 4 lanes read one 64-byte row segment
    auto load_t = [&](const float *P, int ld, int64_t row0, int64_t rows, bool vec, int r, float4v (&dst)[2]) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int q = p * kThreads + tid, row = q >> 2, c4 = (q & 3) * 4;
            dst[p] = (float4v)(0.f);
            if (row0 + row < rows) {
                const float *src = P + (row0 + row) * ld + r + c4;
                if (vec && r + c4 + 3 < R) dst[p] = *(const float4v *)src;
                else
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (r + c4 + e < R) dst[p][e] = src[e];
            }
        }
    };
    auto store_t = [&](float *L, const float4v (&srcv)[2]) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int q = p * kThreads + tid, row = q >> 2, c4 = (q & 3) * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) L[(c4 + e) * 132 + row] = srcv[p][e];
        }
    };
    auto load_stage = [&](int r) {
        load_t(A_, lda, j0, n, va, r, ra);
        if (BT) {
            load_t(B_, ldb, k0, Nc, vb, r, rb);
        } else {
#pragma unroll
            for (int p = 0; p < 2; ++p) {   // natural layout: 16 reduction rows x 32 float4
                const int q = p * kThreads + tid, row = q >> 5, c4 = (q & 31) * 4;
                rb[p] = (float4v)(0.f);
                if (r + row < R) {
                    const float *src = B_ + (int64_t)(r + row) * ldb + k0 + c4;
                    if (vb && k0 + c4 + 3 < Nc) rb[p] = *(const float4v *)src;
                    else
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (k0 + c4 + e < Nc) rb[p][e] = src[e];
                }
            }
        }
    };
    auto store_stage = [&](int buf) {
        store_t(lA[buf], ra);
        if (BT) store_t(lB[buf], rb);
        else
#pragma unroll
            for (int p = 0; p < 2; ++p) *(float4v *)(&lB[buf][(p * kThreads + tid) * 4]) = rb[p];
    };
    load_stage(0);
    store_stage(0);
    __syncthreads();
    int buf = 0;
    for (int r = 0; r < R; r += 16, buf ^= 1) {
        const bool more = r + 16 < R;
        if (more) load_stage(r + 16);
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
            const float a0 = lA[buf][(kk + h) * LDA + wm + li], a1 = lA[buf][(kk + h) * LDA + wm + 32 + li];
            const float b0 = lB[buf][(kk + h) * LDB + wn + li], b1 = lB[buf][(kk + h) * LDB + wn + 32 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (((r >> 4) & (kFold - 1)) == kFold - 1) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int q = 0; q < 16; ++q) { sum[a][b][q] += acc[a][b][q]; acc[a][b][q] = 0.f; }
        }
        if (more) store_stage(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t j = j0 + wm + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const int k = k0 + wn + b * 32 + li;
                if (j < n && k < Nc) {
                    float v = sum[a][b][r] + acc[a][b][r];
                    if (bias) v += bias[k];
                    if (accumulate) v += C[j * ldc + k];
                    C[j * ldc + k] = v;
                }
            }
}

// The register budget is set per variant: with B transposed the body fits 168 registers (3 waves per SIMD); with B in its
// natural layout that cap spills inside the loop (0.92 ms instead of 0.72), so that variant runs at 2 waves per SIMD.
// (blockIdx.y = slice of the reduction, `slice` indices long, whose block goes to C + y * part_stride: launch_gemm_rows_sliced)
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(3, 4))) void gemm_rows_bt_kernel(
    const float *__restrict__ A_, int lda, int64_t n, const float *__restrict__ B_, int ldb, int R, int Nc, float *__restrict__ C, int ldc,
    const float *__restrict__ bias, int accumulate, int slice, int64_t part_stride) {
    const int r0 = blockIdx.y * slice;
    gemm_rows_body<true>(A_ + r0, lda, n, B_ + r0, ldb, slice ? min(slice, R - r0) : R, Nc, C + blockIdx.y * part_stride, ldc, bias, accumulate, slice != 0);
}
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 4))) void gemm_rows_kernel(
    const float *__restrict__ A_, int lda, int64_t n, const float *__restrict__ B_, int ldb, int R, int Nc, float *__restrict__ C, int ldc,
    const float *__restrict__ bias, int accumulate, int slice, int64_t part_stride) {
    const int r0 = blockIdx.y * slice;
    gemm_rows_body<false>(A_ + r0, lda, n, B_ + (int64_t)r0 * ldb, ldb, slice ? min(slice, R - r0) : R, Nc, C + blockIdx.y * part_stride, ldc, bias, accumulate,
                          slice != 0);
}
// C[i] = part[0][i] + part[1][i] + ... in that order (C rows ldc apart, the partial blocks dense [n][Nc])
__global__ __launch_bounds__(kThreads) void gemm_rows_sum_slices_kernel(const float *__restrict__ part, int slices, int64_t n, int Nc, float *__restrict__ C, int ldc) {
    const int64_t total = n * Nc;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        float v = part[i];
        for (int s = 1; s < slices; ++s) v += part[(int64_t)s * total + i];
        C[(i / Nc) * ldc + i % Nc] = v;
    }
}

int launch_gemm_rows(const float *A_, int lda, int64_t n, const float *B_, int ldb, int R, int Nc, float *C, int ldc, bool b_transposed,
                     hipStream_t stream, const float *bias, bool accumulate) {
    if (n <= 0 || Nc <= 0) return MOT_OK;
    if (b_transposed && R > 0 && gemm_rows_f32_256_usable(A_, lda, n, B_, ldb, R, Nc))   // 256 x 256 blocks by LDS-DMA (mot_gemm_bf16.hip)
        return launch_gemm_rows_f32_256(A_, lda, n, B_, ldb, R, Nc, C, ldc, bias, accumulate, stream);
    const int64_t gx = (n + 127) / 128;
    const int gy = (Nc + 127) / 128;
    const int64_t blocks = (gx + 7) / 8 * 8 * gy;   // 1-D, see the block order in the kernel
    if (blocks > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "gemm_rows: too many rows");
    // (one launch covers any R: the kernel sums in blocks)
    if (b_transposed)
        hipLaunchKernelGGL(gemm_rows_bt_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, A_, lda, n, B_, ldb, R, Nc, C, ldc, bias,
                           accumulate ? 1 : 0, 0, (int64_t)0);
    else
        hipLaunchKernelGGL(gemm_rows_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, A_, lda, n, B_, ldb, R, Nc, C, ldc, bias,
                           accumulate ? 1 : 0, 0, (int64_t)0);
    return check_launch("gemm_rows_kernel");
}

// how the reduction of a few-row product is cut: slices of a multiple of 16 indices, at least 64, as many as fill the chip
static int gemm_rows_slices(int64_t n, int R, int Nc, int *slice_len) {
    const int64_t blocks = ((n + 127) / 128 + 7) / 8 * 8 * ((Nc + 127) / 128), live = ((n + 127) / 128) * ((Nc + 127) / 128);
    if (n > 1024 || R < 256 || live >= 128 || blocks > 4096) return 1;
    int want = (int)(768 / live);   // (three workgroups a CU: a step of this kernel is one exposed load latency, ~5 us of it per step measured)
    if (want > R / 64) want = R / 64;
    if (want > 32) want = 32;
    if (want < 2) return 1;
    const int len = ((R + want - 1) / want + 15) / 16 * 16;
    *slice_len = len;
    return (R + len - 1) / len;
}
size_t gemm_rows_sliced_floats(int64_t n, int R, int Nc) {
    int len = 0;
    const int s = gemm_rows_slices(n, R, Nc, &len);
    return s > 1 ? (size_t)s * n * Nc : 0;
}
int launch_gemm_rows_sliced(const float *A_, int lda, int64_t n, const float *B_, int ldb, int R, int Nc, float *C, int ldc, bool b_transposed, float *part,
                            size_t part_floats, hipStream_t stream) {
    int len = 0;
    const int slices = n > 0 && Nc > 0 ? gemm_rows_slices(n, R, Nc, &len) : 1;
    if (slices < 2 || !part || part_floats < (size_t)slices * n * Nc) return launch_gemm_rows(A_, lda, n, B_, ldb, R, Nc, C, ldc, b_transposed, stream);
    const int64_t blocks = ((n + 127) / 128) * ((Nc + 127) / 128);   // (plain block order in the sliced launches: no padded panels)
    const dim3 grid((unsigned)blocks, (unsigned)slices);
    if (b_transposed)
        hipLaunchKernelGGL(gemm_rows_bt_kernel, grid, dim3(kThreads), 0, stream, A_, lda, n, B_, ldb, R, Nc, part, Nc, (const float *)nullptr, 0, len, n * Nc);
    else
        hipLaunchKernelGGL(gemm_rows_kernel, grid, dim3(kThreads), 0, stream, A_, lda, n, B_, ldb, R, Nc, part, Nc, (const float *)nullptr, 0, len, n * Nc);
    if (int rc = check_launch("gemm_rows_kernel")) return rc;
    const int64_t total = n * Nc;
    hipLaunchKernelGGL(gemm_rows_sum_slices_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads < 2048 ? (total + kThreads - 1) / kThreads : 2048)), dim3(kThreads), 0,
                       stream, part, slices, n, Nc, C, ldc);
    return check_launch("gemm_rows_sum_slices_kernel");
}

// dst[c][r] = src[r][c]   (fp32 rows x cols -> cols x rows): a k-major weight as the row-major operand of the LDS-DMA product kernel
__global__ __launch_bounds__(kThreads) void transpose_f32_kernel(const float *__restrict__ src, int rows, int cols, float *__restrict__ dst) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int r = ty; r < 32; r += 8)
        tile[r][tx] = (r0 + r < rows && c0 + tx < cols) ? src[(int64_t)(r0 + r) * cols + c0 + tx] : 0.f;
    __syncthreads();
    for (int c = ty; c < 32; c += 8)
        if (c0 + c < cols && r0 + tx < rows) dst[(int64_t)(c0 + c) * rows + r0 + tx] = tile[tx][c];
}
int launch_transpose_f32(const float *src, int rows, int cols, float *dst, hipStream_t stream) {
    if (rows <= 0 || cols <= 0) return MOT_OK;
    hipLaunchKernelGGL(transpose_f32_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(kThreads), 0, stream, src, rows, cols, dst);
    return check_launch("transpose_f32_kernel");
}

}  // namespace mot
