// mot_ffn_step.hip -- the feed-forward of the character mixer's decode step (mot_ffn_step, gfx950): out = h + w2 (silu(w1 xn) * w3 xn),
// xn = RMSNorm_w(h), for up to 16 rows -- the last line of TokenMixByCharBMMBlock.forward (inference/inference.py:269, 121-144) on
// the rows mot_char_swa_step produced.  Three launches, nothing read on the host, no atomics, every sum in a fixed order:
//   ffn_step_gate   every workgroup stages the R <= 16 normalised rows in LDS (R * dim elements, swa_step_query's arithmetic) and
//                   takes groups of four rows j of w1 TOGETHER with the same rows of w3: a = w1_j xn_r and b = w3_j xn_r come out of
//                   one pass, the staged slice is read from LDS once for both, each weight row is read once.  The lane that holds
//                   the pair stores g[r][j] = silu(a) * b to the workspace.
//   ffn_step_down   g for 16 rows (512 KiB at inter 8192 in fp32) does not fit in LDS, so the reduction over inter is cut into
//                   slices of kFfnSlice elements.  Workgroup (x, y) stages slice y of g and computes that slice's share of 16
//                   columns of w2 g; the shares go to the workspace as fp32.  dim / 4 = 512 wave-sized groups of columns alone
//                   would leave half of the 256 CUs without work; with the slices 1024 workgroups stream w2.
//   ffn_step_sum    out[r][c] = h[r][c] + (the shares of (r, c) added in slice order), per element.  The third launch: closing
//                   the sum inside ffn_step_down would need a counter that is zero before the call (a memset node, or state that
//                   outlives the call), and a workgroup that loops over the slices itself is the half-empty form above.
// The slice length does not depend on the number of rows: a row's bits are the same whatever rows stand beside it.
// MOT_BF16: h, w1, w2, w3 and out are bf16 and read in place; xn, a, silu(a), b, silu(a) * b and the output of w2 are rounded to
// bf16, as the module in a bf16 cast rounds them; sums in fp32; the residual is added to the widened output of w2 in fp32 and the
// sum is rounded once.
#include "mot_step.hpp"

namespace mot {
namespace {

constexpr int kFfnSlice = 1024;   // elements of inter per workgroup of ffn_step_down: 16 rows of fp32 are 64 KiB of LDS

struct FfnArgs {
    int n_rows, dim, inter, slices;
    const void *h, *w1, *w3, *w2;
    const float *norm_w;
    void *g;        // workspace [n_rows, inter], the tensor type
    float *part;    // workspace [slices, n_rows, dim]
    void *out;
    float eps;
};

// step_products for NM matrices in one pass over the staged rows, with weight rows of ld elements of which K are used:
// S_m[r][c] = sum_{k < K} xs[r][k] W[m][c][k] for c in [c0, c0 + 4), the same lane slices, the same order, the same DPP sum;
// f(r, c, S_0 .. S_{NM-1}) is called by lane c - c0 < 4.  (step_products itself takes one matrix whose rows are K long.)
template <typename T, int R, int NM, class F>
__device__ __forceinline__ void ffn_products(const T *__restrict__ xs, const T *const (&W)[NM], int K, int64_t ld, int c0, int n_rows, F &&f) {
    typedef StepVec<T> Vec;
    const int lane = threadIdx.x & 63, kvec = K / Vec::N;
    float acc[NM][kStepCls][R];
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
        for (int c = 0; c < kStepCls; ++c)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[m][c][r] = 0.f;
#pragma unroll 2
    for (int kv = lane; kv < kvec; kv += 64) {
        Vec w[NM][kStepCls];
#pragma unroll
        for (int m = 0; m < NM; ++m)
#pragma unroll
            for (int c = 0; c < kStepCls; ++c) w[m][c] = ((const Vec *)(W[m] + (int64_t)(c0 + c) * ld))[kv];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const Vec xv = ((const Vec *)(xs + r * K))[kv];
#pragma unroll
            for (int e = 0; e < Vec::N; ++e) {
                const float xe = xv.get(e);
#pragma unroll
                for (int m = 0; m < NM; ++m)
#pragma unroll
                    for (int c = 0; c < kStepCls; ++c) acc[m][c][r] = __builtin_fmaf(w[m][c].get(e), xe, acc[m][c][r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float mine[NM];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            float s[kStepCls];
#pragma unroll
            for (int c = 0; c < kStepCls; ++c) s[c] = wave_sum(acc[m][c][r]);
            mine[m] = lane == 0 ? s[0] : lane == 1 ? s[1] : lane == 2 ? s[2] : s[3];
        }
        if (lane < kStepCls && r < n_rows) f(r, c0 + lane, mine);
    }
}

template <typename T, int R>
__global__ __launch_bounds__(kStepThreads) void ffn_step_gate(FfnArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ffn_smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // ---- xn = RMSNorm_w(h) of every row into LDS, as a tensor of type T (swa_step_query's arithmetic)
    T *xs = (T *)ffn_smem;   // [R][dim]
    const int nv = A.dim >> 2;
    for (int r = wave; r < R; r += kStepWaves) {
        T *o = xs + r * A.dim;
        if (r >= A.n_rows) {
            for (int j = lane; j < A.dim; j += 64) o[j] = (T)0.f;
            continue;
        }
        const T *p = (const T *)A.h + (int64_t)r * A.dim;
        float ss = 0.f;
        for (int j = lane; j < nv; j += 64) {
            const float4v v = Elem<T>::load4(p + 4 * j);
            ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
        }
        ss = wave_sum(ss);
        const float rs = 1.0f / sqrtf(ss / (float)A.dim + A.eps);
        for (int j = lane; j < nv; j += 64) {
            const float4v v = Elem<T>::load4(p + 4 * j), w = *(const float4v *)(A.norm_w + 4 * j);
            const float4v x = (v * rs) * w;
            if constexpr (sizeof(T) == 2) *(bf16x4v *)(o + 4 * j) = __builtin_convertvector(x, bf16x4v);
            else *(float4v *)(o + 4 * j) = x;
        }
    }
    __syncthreads();
    // ---- g = silu(w1 xn) * w3 xn: groups of four rows of w1 and of w3, one group per wave at a time
    const int groups = A.inter / kStepCls;
    const T *const W[2] = {(const T *)A.w1, (const T *)A.w3};
    for (int g = blockIdx.x * kStepWaves + wave; g < groups; g += gridDim.x * kStepWaves)
        ffn_products<T, R, 2>(xs, W, A.dim, A.dim, g * kStepCls, A.n_rows, [&](int r, int j, const float (&s)[2]) {
            const float a = step_round<T>(s[0]), b = step_round<T>(s[1]);
            // silu as a quotient: exp(-a) = inf for a < -88.8 gives -0, never inf * 0
            const float sl = step_round<T>(a / (1.0f + expf(-a)));
            Elem<T>::store1((T *)A.g + (int64_t)r * A.inter + j, sl * b);
        });
}

// workgroup (x, y): columns [16 x, 16 x + 16) of w2 against slice y of g -> part[y]
template <typename T, int R>
__global__ __launch_bounds__(kStepThreads) void ffn_step_down(FfnArgs A) {
    typedef StepVec<T> Vec;
    extern __shared__ __attribute__((aligned(16))) unsigned char ffn_smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int slice = blockIdx.y, k0 = slice * kFfnSlice, len = min(kFfnSlice, A.inter - k0), lv = len / Vec::N;
    Vec *gs = (Vec *)ffn_smem;   // [R][len]
    for (int i = threadIdx.x; i < R * lv; i += kStepThreads) {
        const int r = i / lv, v = i - r * lv;
        gs[i] = r < A.n_rows ? ((const Vec *)((const T *)A.g + (int64_t)r * A.inter + k0))[v] : Vec{};
    }
    __syncthreads();
    const int g = blockIdx.x * kStepWaves + wave;
    if (g >= A.dim / kStepCls) return;
    const T *const W[1] = {(const T *)A.w2 + k0};
    float *part = A.part + (int64_t)slice * A.n_rows * A.dim;
    ffn_products<T, R, 1>((const T *)gs, W, len, A.inter, g * kStepCls, A.n_rows,
                          [&](int r, int c, const float (&s)[1]) { part[(int64_t)r * A.dim + c] = s[0]; });
}

// out = h + (the output of w2: the slices' shares in slice order, a value of a tensor of type T); one thread per four columns
template <typename T>
__global__ __launch_bounds__(kThreads) void ffn_step_sum(FfnArgs A) {
    const int64_t i = 4 * ((int64_t)blockIdx.x * kThreads + threadIdx.x), n = (int64_t)A.n_rows * A.dim;
    if (i >= n) return;
    float4v y = *(const float4v *)(A.part + i);
    for (int s = 1; s < A.slices; ++s) y += *(const float4v *)(A.part + s * n + i);
    const float4v hv = Elem<T>::load4((const T *)A.h + i);
    const float4v x = float4v{step_round<T>(y.x), step_round<T>(y.y), step_round<T>(y.z), step_round<T>(y.w)} + hv;
    if constexpr (sizeof(T) == 2) *(bf16x4v *)((T *)A.out + i) = __builtin_convertvector(x, bf16x4v);
    else *(float4v *)((T *)A.out + i) = x;
}

struct FfnGeom {
    int R, slices;
    bool bf16;
    size_t g, part, total;   // workspace offsets in bytes
};

// every refusal of the call but the workspace's, before any HIP call (the size query makes the same checks)
int ffn_check(const MotFfnStepDesc *d, FfnGeom *out, const char *fn) {
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotFfnStepDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotFfnStepDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EINVAL, "%s: bad dtype %d", fn, d->dtype);
    if (d->reserved0 || d->reserved1 || d->reserved2) return set_error(MOT_EINVAL, "%s: reserved fields must be 0", fn);
    if (d->n_rows < 1 || d->n_rows > kStepMaxRows)
        return set_error(MOT_EUNSUPPORTED, "%s: n_rows %d outside 1..%d: the step is built for a few rows, use the torch path (FeedForward)", fn,
                         d->n_rows, kStepMaxRows);
    if (d->dim < 4 || (d->dim & 3) || d->inter < 4 || (d->inter & 3) || d->inter > (1 << 24))
        return set_error(MOT_ESHAPE, "%s: dim %d / inter %d (multiples of 4, inter at most 2^24)", fn, d->dim, d->inter);
    if (d->dtype == MOT_BF16 && ((d->dim & 7) || (d->inter & 7)))
        return set_error(MOT_EUNSUPPORTED, "%s: bf16 needs dim %d and inter %d to be multiples of 8", fn, d->dim, d->inter);
    FfnGeom &g = *out;
    g.bf16 = d->dtype == MOT_BF16;
    g.R = d->n_rows <= 1 ? 1 : d->n_rows <= 2 ? 2 : d->n_rows <= 4 ? 4 : d->n_rows <= 8 ? 8 : 16;
    g.slices = (d->inter + kFfnSlice - 1) / kFfnSlice;
    const size_t e = g.bf16 ? 2 : 4;
    if ((size_t)g.R * d->dim * e > kStepMaxLds)
        return set_error(MOT_EUNSUPPORTED, "%s: %d rows x %d elements need more than %zu B of LDS, use the torch path (FeedForward)", fn, g.R,
                         d->dim, kStepMaxLds);
    if (!d->h || !d->norm_w || !d->w1 || !d->w3 || !d->w2 || !d->out) return set_error(MOT_EINVAL, "%s: h/norm_w/w1/w3/w2/out must be non-null", fn);
    if (((uintptr_t)d->h & 15) || ((uintptr_t)d->norm_w & 15) || ((uintptr_t)d->w1 & 15) || ((uintptr_t)d->w3 & 15) || ((uintptr_t)d->w2 & 15) ||
        ((uintptr_t)d->out & 15))
        return set_error(MOT_EUNSUPPORTED, "%s: h, norm_w, the weights and out must be 16-byte aligned", fn);
    const uintptr_t hb = (uintptr_t)d->h, ob = (uintptr_t)d->out, bytes = (uintptr_t)d->n_rows * d->dim * e;
    if (hb < ob + bytes && ob < hb + bytes)
        return set_error(MOT_EINVAL, "%s: out overlaps h (every workgroup reads all of h while others write out)", fn);
    Arena a;
    g.g = a.take((size_t)d->n_rows * d->inter * e);
    g.part = a.take((size_t)g.slices * d->n_rows * d->dim * sizeof(float));
    g.total = a.o;
    return MOT_OK;
}

template <typename T, int R>
int ffn_run(const FfnArgs &A, hipStream_t stream) {
    static std::atomic<uint64_t> lds_g{0}, lds_d{0};
    const size_t lg = (size_t)R * A.dim * sizeof(T), ld = (size_t)R * (A.inter < kFfnSlice ? A.inter : kFfnSlice) * sizeof(T);
    if (lg > (48u << 10))
        if (int rc = ensure_max_dyn_lds((const void *)ffn_step_gate<T, R>, lds_g, "ffn_step_gate")) return rc;
    if (ld > (48u << 10))
        if (int rc = ensure_max_dyn_lds((const void *)ffn_step_down<T, R>, lds_d, "ffn_step_down")) return rc;
    const int gblocks = (A.inter / kStepCls + kStepWaves - 1) / kStepWaves, dblocks = (A.dim / kStepCls + kStepWaves - 1) / kStepWaves;
    hipLaunchKernelGGL((ffn_step_gate<T, R>), dim3((unsigned)gblocks), dim3(kStepThreads), lg, stream, A);
    if (int rc = check_launch("ffn_step_gate")) return rc;
    hipLaunchKernelGGL((ffn_step_down<T, R>), dim3((unsigned)dblocks, (unsigned)A.slices), dim3(kStepThreads), ld, stream, A);
    if (int rc = check_launch("ffn_step_down")) return rc;
    const int64_t quads = (int64_t)A.n_rows * A.dim / 4;
    hipLaunchKernelGGL((ffn_step_sum<T>), dim3((unsigned)((quads + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, A);
    return check_launch("ffn_step_sum");
}

template <typename T>
int ffn_rows(const FfnArgs &A, int R, hipStream_t stream) {
    return R == 1 ? ffn_run<T, 1>(A, stream)
         : R == 2 ? ffn_run<T, 2>(A, stream)
         : R == 4 ? ffn_run<T, 4>(A, stream)
         : R == 8 ? ffn_run<T, 8>(A, stream)
                  : ffn_run<T, 16>(A, stream);
}

}  // namespace

size_t ffn_step_workspace_bytes(const MotFfnStepDesc *d) {
    FfnGeom g;
    if (ffn_check(d, &g, "mot_ffn_step_workspace_bytes")) return 0;
    return g.total;
}

int launch_ffn_step(const MotFfnStepDesc *d, hipStream_t stream) {
    static const char fn[] = "mot_ffn_step";
    FfnGeom g;
    if (int rc = ffn_check(d, &g, fn)) return rc;
    if (int rc = check_workspace(fn, false, d->workspace, d->workspace_bytes, g.total)) return rc;
    FfnArgs A{};
    A.n_rows = d->n_rows; A.dim = d->dim; A.inter = d->inter; A.slices = g.slices;
    A.h = d->h; A.w1 = d->w1; A.w3 = d->w3; A.w2 = d->w2; A.norm_w = d->norm_w;
    A.g = (unsigned char *)d->workspace + g.g; A.part = (float *)((unsigned char *)d->workspace + g.part);
    A.out = d->out;
    A.eps = d->norm_eps > 0.f ? d->norm_eps : 1e-5f;
    return g.bf16 ? ffn_rows<__bf16>(A, g.R, stream) : ffn_rows<float>(A, g.R, stream);
}

}  // namespace mot
