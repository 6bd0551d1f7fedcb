// mot_headstep.hip -- mot_byte_head_step: the split-mode byte head's training step (mot_head.hip's forward and backward with
// grad_loss = 1) in one call.  bf16 first (the fp32 form is described at its kernel): a persistent grid of kStepGrid workgroups,
// each holding W in LDS, walks tiles of kStepTileRows byte rows; a wave owns 32 rows.  The logits are formed TRANSPOSED, S^T[class][row] = W x^T on v_mfma_f32_32x32x16_bf16, so a row
// sits on a lane (and its partner lane ^ 32) and the classes in accumulator registers: c, the cap, sum exp(z - 30), the target's z
// and G = c (1 / M) 4 s (1 - s) (p - onehot) are register work, and u^T[k][row] = W^T G^T sums over G's register index, so the
// accumulator tile, packed to bf16, is that product's B operand with no lane movement.  The 16 class tiles of 32 are walked twice
// (sum, then gradient) on one 16-register accumulator.  Nothing 512 wide per row goes to memory on the way to loss and dx.
// dW = G^T x sums over the lane index: the kernel stores the chunk's G in bf16 (1 KB a row) and the shared launch_gemm_tn_bf16 adds
// the chunk into dW (fp32 atomics) behind a launch_zero_words.
//
// k orders.  An accumulator tile of 32x32x16 holds, in register i of lane half h, row 8 (i >> 2) + 4 h + (i & 3): as an operand of
// the next product its element j of k-step s is row 16 s + 8 (j >> 2) + 4 h + (j & 3).  Both LDS images are laid out in that order,
// so that every fragment is one 16-byte read:
//   Wk [class][K + 8]:  element 16 ks + 8 h + j  =  W[class][16 ks + 8 (j >> 2) + 4 h + (j & 3)]   (A of S^T = W x^T)
//   Wc [k][512 + 8]:    element 32 ct + 16 s + 8 h + j  =  W[32 ct + 16 s + 8 (j >> 2) + 4 h + (j & 3)][k]   (A of u^T = W^T G^T)
// and a lane's x fragments use the same k order, which is the order of its u accumulators: x . u and the chain are lane-local
// but for one exchange with lane ^ 32.  The row stride of both images is 4 (mod 8) dwords: 16-byte reads without bank conflicts.
// Wc comes from one prep kernel into the workspace ([Kp][520], Kp = K rounded up to 32, zero rows behind K); it is copied to LDS
// where both images fit (K <= 64) and read through L2 above that.
#include "mot_headcore.hpp"

namespace mot {
namespace {

constexpr int kV = 512;
constexpr int kStepThreads = 512;                       // 8 waves: two a SIMD, one workgroup a CU (the LDS images)
constexpr int kStepTileRows = kStepThreads / 64 * 32;   // 256 byte rows a tile
constexpr int kStepGrid = 256;                          // persistent workgroups: min(tiles, kStepGrid), from the shape alone
constexpr int64_t kStepChunkRows = 131072;              // rows of G in the workspace: two tiles a workgroup; 128 MiB in bf16, 256 in fp32
constexpr int kStepMaxK = 128, kStepLdsWcMaxK = 64;     // bf16: W (K + 8 wide) must fit in 160 KiB; beside Wc (Kp x 520) up to K = 64
constexpr int kStepMaxKF = 64;                          // fp32: W (K + 1 wide) is 130 KiB at K = 64
constexpr int kWcLd = kV + 8;
constexpr float kCap = 30.f, kInvDiv = 1.f / 7.5f;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float sigm(float l) { return 1.f / (1.f + __expf(-l * kInvDiv)); }
__device__ __forceinline__ float pair_sum(float v) { return v + __shfl_xor(v, 32, 64); }   // with the row's other lane: the same bits on both

struct StepArgs {
    const void *x, *W, *Wc;   // in dtype; Wc: the class-ordered k-major image in the workspace (bf16 only)
    void *aux;                // fp32, TRAIN only: the chunk's rows of x / se
    const int64_t *tgt;
    int64_t rows;   // of this launch
    int L;
    float eps, inv_m;
    float *term;
    uint32_t *status;
    void *G, *dx;   // TRAIN only, in dtype
};

// Wc[k][p] for p < 512, zero behind K and in the pad
__global__ __launch_bounds__(kThreads) void head_step_wc(const __bf16 *__restrict__ W, int K, int Kp, __bf16 *__restrict__ Wc) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= Kp * kWcLd) return;
    const int k = idx / kWcLd, p = idx - k * kWcLd;
    __bf16 v = (__bf16)0.f;
    if (k < K && p < kV) {
        const int q = p & 15, h = (q >> 3) & 1, j = q & 7;
        v = W[(int64_t)((p & ~15) + 8 * (j >> 2) + 4 * h + (j & 3)) * K + k];
    }
    Wc[idx] = v;
}

// KS = K / 16 k-steps of the first product; KT = ceil(KS / 2) tiles of 32 k in u
template <int KS, bool TRAIN>
__global__ __launch_bounds__(kStepThreads) void head_step_kernel(StepArgs a) {
    constexpr int K = 16 * KS, KT = (KS + 1) / 2, ldk = K + 8;
    constexpr bool WC_LDS = K <= kStepLdsWcMaxK;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const __bf16 *ax = (const __bf16 *)a.x, *aW = (const __bf16 *)a.W, *aWc = (const __bf16 *)a.Wc;
    __bf16 *Wk = (__bf16 *)smem;
    __bf16 *WcL = Wk + kV * ldk;
    for (int i = threadIdx.x; i < kV * KS; i += kStepThreads) {   // 16 elements of a row of W: quads 0 2 1 3
        const int cls = i / KS, ks = i - cls * KS;
        const uint2 *src = (const uint2 *)(aW + (int64_t)cls * K + 16 * ks);
        const uint2 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
        uint4 *dst = (uint4 *)(Wk + cls * ldk + 16 * ks);
        dst[0] = make_uint4(q0.x, q0.y, q2.x, q2.y);
        dst[1] = make_uint4(q1.x, q1.y, q3.x, q3.y);
    }
    if (TRAIN && WC_LDS)
        for (int i = threadIdx.x; i < 32 * KT * kWcLd / 8; i += kStepThreads) ((uint4 *)WcL)[i] = ((const uint4 *)aWc)[i];
    __syncthreads();

    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    const int64_t tiles = (a.rows + kStepTileRows - 1) / kStepTileRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = tile * kStepTileRows + wave * 32 + r;
        const bool live = row < a.rows;
        // the row's half of x in the k order of the images: fragment ks, elements j = 0..3 | 4..7 are x[16 ks + 4 h ..] | x[16 ks + 8 + 4 h ..]
        bf16x8 xf[KS];
        float ss = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            uint2 lo = make_uint2(0u, 0u), hi = lo;
            if (live) {
                const uint2 *p = (const uint2 *)(ax + row * K + 16 * ks + 4 * h);
                lo = p[0];
                hi = p[2];
            }
            xf[ks] = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = (float)xf[ks][j];
                ss += v * v;
            }
        }
        ss = pair_sum(ss);
        float c, dc;
        row_scale(ss / (float)K, a.L, a.eps, c, dc);
        const int64_t y64 = live ? a.tgt[row] : -1;
        const bool in = y64 >= 0 && y64 < kV;   // an out-of-range target addresses nothing
        const int y = in ? (int)y64 : -1;

        // pass 1: sum exp(z - 30) and the target's z
        float se = 0.f, tz = 0.f;
#pragma unroll 1
        for (int ct = 0; ct < kV / 32; ++ct) {
            f32x16 s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8 *)(Wk + (32 * ct + r) * ldk + 16 * ks + 8 * h), xf[ks], s, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float z = kCap * sigm(c * s[i]);
                se += __expf(z - kCap);
                tz += (32 * ct + 8 * (i >> 2) + 4 * h + (i & 3) == y) ? z : 0.f;
            }
        }
        se = pair_sum(se);
        tz = pair_sum(tz);
        const float lse = kCap + __logf(se);
        if (live && h == 0) {
            a.term[row] = in ? lse - tz : 0.f;
            if (!in && a.status) atomicOr(a.status, (uint32_t)MOT_STATUS_TARGET_OOR);
        }
        if constexpr (TRAIN) {

        // pass 2: the same logits again, G into the fragment of u^T = W^T G^T and into the chunk's G for dW
        const float nv = in ? 1.f : 0.f;
        f32x16 u[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) u[kt] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int ct = 0; ct < kV / 32; ++ct) {
            f32x16 s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8 *)(Wk + (32 * ct + r) * ldk + 16 * ks + 8 * h), xf[ks], s, 0, 0, 0);
            bf16x8 gf[2];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float sg = sigm(c * s[i]), z = kCap * sg, p = __expf(z - lse);
                const float hit = (32 * ct + 8 * (i >> 2) + 4 * h + (i & 3) == y) ? 1.f : 0.f;
                const float g = a.inv_m * 4.f * sg * (1.f - sg) * (nv * p - hit);
                gf[i >> 3][i & 7] = (__bf16)(c * g);   // rounded once, for both products that take it
            }
            if (live) {   // registers 4 g .. 4 g + 3 are classes 32 ct + 8 g + 4 h ..
                __bf16 *gr = (__bf16 *)a.G + row * kV + 32 * ct + 4 * h;
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *(bf16x4 *)(gr + 8 * g4) = bf16x4{gf[g4 >> 1][4 * (g4 & 1)], gf[g4 >> 1][4 * (g4 & 1) + 1], gf[g4 >> 1][4 * (g4 & 1) + 2], gf[g4 >> 1][4 * (g4 & 1) + 3]};
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) {
                    const int at = (32 * kt + r) * kWcLd + 32 * ct + 16 * s2 + 8 * h;
                    const bf16x8 wf = WC_LDS ? *(const bf16x8 *)(WcL + at) : *(const bf16x8 *)(aWc + at);
                    u[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf, gf[s2], u[kt], 0, 0, 0);
                }
        }
        // u[kt][i] is k = 32 kt + 8 (i >> 2) + 4 h + (i & 3), which is element i & 7 of x fragment 2 kt + (i >> 3)
        float xu = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (2 * kt + (i >> 3) < KS) xu += (float)xf[2 * kt + (i >> 3)][i & 7] * u[kt][i];
        xu = pair_sum(xu);
        // the chain of head_chain_rows: a row that is zero to fp32's sum of squares has dx = u
        const float m0 = ss / (float)K;
        const float coef = m0 > 0.f ? (float)(row_scale_dlog((double)m0, a.L, (double)a.eps) * (2.0 / (double)K) * (double)xu) : 0.f;
        if (live) {
            __bf16 *dr = (__bf16 *)a.dx + row * K + 4 * h;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    if (2 * kt + (g4 >> 1) < KS) {
                        bf16x4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int i = 4 * g4 + e;
                            o[e] = (__bf16)(u[kt][i] + coef * (float)xf[2 * kt + (i >> 3)][i & 7]);
                        }
                        *(bf16x4 *)(dr + 32 * kt + 8 * g4) = o;
                    }
        }
        }   // TRAIN
    }
}

// The fp32 form: v_mfma_f32_32x32x2_f32, whose operands are one float a lane (A[i = lane & 31][k = lane >> 5], B likewise), so ONE
// row-major image of W in LDS ([512][K + 1]: an odd stride, every read conflict-free) serves both products: S^T reads W[class = lane][k]
// and u^T reads W[class][k = lane].  A lane holds x at the k of its u accumulators (k = 32 kt + 8 g + 4 h + e), and the first product
// pairs its two k slots accordingly.  A tile's logits are formed ONCE, on one 16-register accumulator, and nothing waits for the
// row's sum: with e = exp(z - 30), se = sum e and a = 4 s (1 - s), G = c (1 / M) a (e / se - onehot) = G' / se with
// G' = c (1 / M) a (e - onehot se).  The walk stores G' without the target's term and sums u'' = G' W on the MFMA; once se is known
// the one element G'[y] is stored again by the lane that wrote it, u = u'' / se - c (1 / M) a_y W[y], and the row's x / se goes to the
// workspace, so that dW = G^T x = G'^T (x / se) is the shared product over what the kernel stored.
template <int KS, bool TRAIN>
__global__ __launch_bounds__(kStepThreads) void head_step_f32_kernel(StepArgs a) {
    constexpr int K = 16 * KS, KT = (KS + 1) / 2, ldw = K + 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *Wl = (float *)smem;   // kV * ldw floats and 32 more: u's rows behind K read past a row's end
    const float *ax = (const float *)a.x, *aW = (const float *)a.W;
    for (int i = threadIdx.x; i < kV * K / 4; i += kStepThreads) {
        const float4 v = ((const float4 *)aW)[i];
        const int cls = (4 * i) / K, k = 4 * i - cls * K;
        float *dst = Wl + cls * ldw + k;
        dst[0] = v.x;
        dst[1] = v.y;
        dst[2] = v.z;
        dst[3] = v.w;
    }
    if (threadIdx.x < 32) Wl[kV * ldw + threadIdx.x] = 0.f;
    __syncthreads();

    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    const int64_t tiles = (a.rows + kStepTileRows - 1) / kStepTileRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row = tile * kStepTileRows + wave * 32 + r;
        const bool live = row < a.rows;
        f32x16 xv[KT];   // xv[kt][4 g + e] = x[32 kt + 8 g + 4 h + e]: the k of u[kt][4 g + e]
        float ss = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (2 * kt + (g4 >> 1) < KS && live) v = *(const float4 *)(ax + row * K + 32 * kt + 8 * g4 + 4 * h);
                xv[kt][4 * g4] = v.x;
                xv[kt][4 * g4 + 1] = v.y;
                xv[kt][4 * g4 + 2] = v.z;
                xv[kt][4 * g4 + 3] = v.w;
                ss += v.x * v.x;
                ss += v.y * v.y;
                ss += v.z * v.z;
                ss += v.w * v.w;
            }
        ss = pair_sum(ss);
        float c, dc;
        row_scale(ss / (float)K, a.L, a.eps, c, dc);
        const int64_t y64 = live ? a.tgt[row] : -1;
        const bool in = y64 >= 0 && y64 < kV;   // an out-of-range target addresses nothing: its row of G is zero
        const int y = in ? (int)y64 : -1;
        const float gs = in ? c * a.inv_m : 0.f;

        float se = 0.f, tz = 0.f, ay = 0.f;
        f32x16 u[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) u[kt] = f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int ct = 0; ct < kV / 32; ++ct) {
            f32x16 s = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const float *wr = Wl + (32 * ct + r) * ldw + 4 * h;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (2 * kt + (i >> 3) < KS) s = __builtin_amdgcn_mfma_f32_32x32x2f32(wr[32 * kt + 8 * (i >> 2) + (i & 3)], xv[kt][i], s, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) {   // register i is class 32 ct + 8 (i >> 2) + 4 h + (i & 3)
                const float sg = sigm(c * s[i]), z = kCap * sg, e = __expf(z - kCap);
                const bool hit = 32 * ct + 8 * (i >> 2) + 4 * h + (i & 3) == y;
                se += e;
                tz += hit ? z : 0.f;
                if (TRAIN) {
                    const float av = 4.f * sg * (1.f - sg);
                    ay += hit ? av : 0.f;
                    s[i] = gs * av * e;
                }
            }
            if constexpr (TRAIN) {
                if (live) {
                    float *gr = (float *)a.G + row * kV + 32 * ct + 4 * h;
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4) *(float4 *)(gr + 8 * g4) = make_float4(s[4 * g4], s[4 * g4 + 1], s[4 * g4 + 2], s[4 * g4 + 3]);
                }
                const float *wc = Wl + (32 * ct + 4 * h) * ldw + r;
#pragma unroll
                for (int i = 0; i < 16; ++i)
#pragma unroll
                    for (int kt = 0; kt < KT; ++kt)
                        u[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(wc[(8 * (i >> 2) + (i & 3)) * ldw + 32 * kt], s[i], u[kt], 0, 0, 0);
            }
        }
        se = pair_sum(se);
        tz = pair_sum(tz);   // one term in the pair is the target's z, the rest are zeros: exact
        const float lse = kCap + __logf(se);
        if (live && h == 0) {
            a.term[row] = in ? lse - tz : 0.f;
            if (!in && a.status) atomicOr(a.status, (uint32_t)MOT_STATUS_TARGET_OOR);
        }
        if constexpr (TRAIN) {
            ay = pair_sum(ay);
            const float inv_se = 1.f / se, gy = gs * ay;
            // the target's element again, with its term, from the lane that stored it in the walk
            if (in && h == ((y >> 2) & 1)) ((float *)a.G)[row * kV + y] = gy * (__expf(tz - kCap) - se);
            const float *wy = Wl + (in ? y : 0) * ldw + 4 * h;
            float xu = 0.f;   // rows of u behind K hold products with whatever lies behind W's row: never read
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (2 * kt + (i >> 3) < KS) {
                        u[kt][i] = u[kt][i] * inv_se - gy * wy[32 * kt + 8 * (i >> 2) + (i & 3)];
                        xu += xv[kt][i] * u[kt][i];
                    }
            xu = pair_sum(xu);
            // the chain of head_chain_rows: a row that is zero to fp32's sum of squares has dx = u
            const float m0 = ss / (float)K;
            const float coef = m0 > 0.f ? (float)(row_scale_dlog((double)m0, a.L, (double)a.eps) * (2.0 / (double)K) * (double)xu) : 0.f;
            if (live) {
                float *dr = (float *)a.dx + row * K + 4 * h, *xs = (float *)a.aux + row * K + 4 * h;
#pragma unroll
                for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                    for (int g4 = 0; g4 < 4; ++g4)
                        if (2 * kt + (g4 >> 1) < KS) {
                            const int i = 4 * g4;
                            *(float4 *)(dr + 32 * kt + 8 * g4) = make_float4(u[kt][i] + coef * xv[kt][i], u[kt][i + 1] + coef * xv[kt][i + 1],
                                                                             u[kt][i + 2] + coef * xv[kt][i + 2], u[kt][i + 3] + coef * xv[kt][i + 3]);
                            *(float4 *)(xs + 32 * kt + 8 * g4) =
                                make_float4(xv[kt][i] * inv_se, xv[kt][i + 1] * inv_se, xv[kt][i + 2] * inv_se, xv[kt][i + 3] * inv_se);
                        }
            }
        }
    }
}

struct StepGeom {
    int64_t rows;    // byte rows: n_tokens * bpt
    int64_t chunk;   // rows of G in the workspace, one fused launch each: two tiles a workgroup of the full grid
    int K, Kp;
    bool bf16;
    float eps;
};

struct StepWs {   // carve of the workspace, offsets in bytes
    size_t term, part, aux, G, total;   // aux: bf16 the class-ordered k-major W; fp32 a chunk's rows of x / se
};

StepWs step_ws(const StepGeom &g) {
    Arena a;
    StepWs w{};
    w.term = a.take((size_t)g.rows * 4);                                             // the loss's per-row terms
    w.part = a.take((size_t)kLossParts * 8);                                         // its partial sums
    const size_t chunk = (size_t)(g.rows < g.chunk ? g.rows : g.chunk);
    w.aux = a.take(g.bf16 ? (size_t)g.Kp * kWcLd * 2 : chunk * g.K * 4);
    w.G = a.take(chunk * kV * (g.bf16 ? 2 : 4));                                     // a chunk's G in dtype (fp32: G se)
    w.total = a.o;
    return w;
}

// every check the descriptor alone allows, in the order of include/mot.h; *g is set on MOT_OK
int step_geom(const MotByteHeadDesc *d, StepGeom *g) {
    static const char fn[] = "byte_head_step";
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotByteHeadDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotByteHeadDesc));
    if (d->method != MOT_HEAD_SPLIT)
        return set_error(MOT_EUNSUPPORTED, "%s: method %d: only split mode is built here (copy mode's weight does not fit in LDS: use mot_byte_head_fwd / _bwd)", fn,
                         d->method);
    if (d->vocab != kV) return set_error(MOT_EUNSUPPORTED, "%s: vocab %d: only the %d-row head is built", fn, d->vocab, kV);
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EUNSUPPORTED, "%s: dtype %d is not built", fn, d->dtype);
    if (d->n_tokens < 0 || d->model_dim <= 0 || d->n_layer_out < 0 || d->n_layer_out > 64)
        return set_error(MOT_ESHAPE, "%s: n_tokens %lld, model_dim %d, n_layer_out %d", fn, (long long)d->n_tokens, d->model_dim, d->n_layer_out);
    if (d->bpt < 1 || d->bpt > MOT_MAX_BPT) return set_error(MOT_ESHAPE, "%s: bpt %d outside [1, %d]", fn, d->bpt, MOT_MAX_BPT);
    if (d->model_dim % d->bpt)
        return set_error(MOT_ESHAPE, "%s: split needs model_dim %% bpt == 0 (train_gpt.py:503), got %d %% %d", fn, d->model_dim, d->bpt);
    const bool bf16 = d->dtype == MOT_BF16;
    const int K = d->model_dim / d->bpt, max_k = bf16 ? kStepMaxK : kStepMaxKF;
    if (K % 16 || K > max_k)
        return set_error(MOT_EUNSUPPORTED, "%s: row width %d must be a multiple of 16 and at most %d in this dtype: W and its staging must fit in LDS", fn, K,
                         max_k);
    const int64_t M = d->n_tokens * (int64_t)d->bpt;
    if (M > (1ll << 31)) return set_error(MOT_EUNSUPPORTED, "%s: n_tokens * bpt exceeds 2^31", fn);
    if (!d->x || !d->weight || !d->targets || !d->loss) return set_error(MOT_EINVAL, "%s: null x / weight / targets / loss", fn);
    if (((uintptr_t)d->x & 15) || ((uintptr_t)d->weight & 15)) return set_error(MOT_EUNSUPPORTED, "%s: x, weight and dx must be 16-byte aligned", fn);
    if (M == 0) return set_error(MOT_ESHAPE, "%s: no targets (the mean over zero targets is undefined)", fn);
    g->rows = M;
    g->chunk = kStepChunkRows;
    g->K = K;
    g->Kp = (K + 31) / 32 * 32;
    g->bf16 = bf16;
    g->eps = d->eps > 0.f ? d->eps : kHeadEps;
    return MOT_OK;
}

template <int KS, bool TRAIN>
int step_launch(const StepArgs &a, hipStream_t stream) {
    constexpr int K = 16 * KS, KT = (KS + 1) / 2;
    const size_t lds = (size_t)kV * (K + 8) * 2 + (TRAIN && K <= kStepLdsWcMaxK ? (size_t)32 * KT * kWcLd * 2 : 0);
    static std::atomic<uint64_t> lds_ok{0};   // per-device bits
    if (int rc = ensure_max_dyn_lds((const void *)head_step_kernel<KS, TRAIN>, lds_ok, "head_step_kernel")) return rc;
    const int64_t tiles = (a.rows + kStepTileRows - 1) / kStepTileRows;
    hipLaunchKernelGGL((head_step_kernel<KS, TRAIN>), dim3((unsigned)(tiles < kStepGrid ? tiles : kStepGrid)), dim3(kStepThreads), lds, stream, a);
    return check_launch("head_step_kernel");
}

template <int KS, bool TRAIN>
int step_launch_f32(const StepArgs &a, hipStream_t stream) {
    const size_t lds = ((size_t)kV * (16 * KS + 1) + 32) * 4;
    static std::atomic<uint64_t> lds_ok{0};   // per-device bits
    if (int rc = ensure_max_dyn_lds((const void *)head_step_f32_kernel<KS, TRAIN>, lds_ok, "head_step_f32_kernel")) return rc;
    const int64_t tiles = (a.rows + kStepTileRows - 1) / kStepTileRows;
    hipLaunchKernelGGL((head_step_f32_kernel<KS, TRAIN>), dim3((unsigned)(tiles < kStepGrid ? tiles : kStepGrid)), dim3(kStepThreads), lds, stream, a);
    return check_launch("head_step_f32_kernel");
}

template <bool TRAIN>
int step_launch_k(bool bf16, int K, const StepArgs &a, hipStream_t stream) {
    if (!bf16) switch (K / 16) {
        case 1: return step_launch_f32<1, TRAIN>(a, stream);
        case 2: return step_launch_f32<2, TRAIN>(a, stream);
        case 3: return step_launch_f32<3, TRAIN>(a, stream);
        case 4: return step_launch_f32<4, TRAIN>(a, stream);
    }
    else switch (K / 16) {
        case 1: return step_launch<1, TRAIN>(a, stream);
        case 2: return step_launch<2, TRAIN>(a, stream);
        case 3: return step_launch<3, TRAIN>(a, stream);
        case 4: return step_launch<4, TRAIN>(a, stream);
        case 5: return step_launch<5, TRAIN>(a, stream);
        case 6: return step_launch<6, TRAIN>(a, stream);
        case 7: return step_launch<7, TRAIN>(a, stream);
        case 8: return step_launch<8, TRAIN>(a, stream);
    }
    return set_error(MOT_EUNSUPPORTED, "byte_head_step: row width %d", K);
}

}  // namespace

size_t byte_head_step_workspace_bytes(const MotByteHeadDesc *d) {
    StepGeom g;
    return step_geom(d, &g) ? 0 : step_ws(g).total;
}

int launch_byte_head_step(const MotByteHeadDesc *d, void *dx, float *dW, hipStream_t stream) {
    static const char fn[] = "byte_head_step";
    StepGeom g;
    int rc = step_geom(d, &g);
    if (rc) return rc;
    if (!dx != !dW) return set_error(MOT_EINVAL, "%s: dx and dW come together (both NULL: the loss alone)", fn);
    if ((uintptr_t)dx & 15) return set_error(MOT_EUNSUPPORTED, "%s: x, weight and dx must be 16-byte aligned", fn);
    const StepWs w = step_ws(g);
    if (!d->workspace || d->workspace_bytes < w.total)
        return set_error(MOT_EWORKSPACE, "%s: workspace %zu bytes < %zu", fn, d->workspace ? d->workspace_bytes : (size_t)0, w.total);
    unsigned char *ws = (unsigned char *)d->workspace;
    float *term = (float *)(ws + w.term);
    const size_t elem = g.bf16 ? 2 : 4;
    StepArgs a{};
    a.W = d->weight;
    a.Wc = a.aux = ws + w.aux;
    a.L = d->n_layer_out;
    a.eps = g.eps;
    a.inv_m = (float)(1.0 / (double)g.rows);
    a.status = d->status;
    if (!dx) {   // the loss alone: one launch over every row, nothing per logit
        a.x = d->x;
        a.tgt = d->targets;
        a.rows = g.rows;
        a.term = term;
        if ((rc = step_launch_k<false>(g.bf16, g.K, a, stream))) return rc;
        return launch_head_loss(term, g.rows, (double *)(ws + w.part), 1.0 / (double)g.rows, d->loss, stream);
    }
    if (g.bf16) {
        hipLaunchKernelGGL(head_step_wc, dim3((unsigned)((g.Kp * kWcLd + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, (const __bf16 *)d->weight, g.K,
                           g.Kp, (__bf16 *)(ws + w.aux));
        if ((rc = check_launch("head_step_wc"))) return rc;
    }
    if ((rc = launch_zero_words(dW, (int64_t)kV * g.K, stream))) return rc;
    a.G = ws + w.G;
    for (int64_t r0 = 0; r0 < g.rows; r0 += g.chunk) {
        const int64_t n = g.rows - r0 < g.chunk ? g.rows - r0 : g.chunk;
        a.x = (const unsigned char *)d->x + (size_t)r0 * g.K * elem;
        a.tgt = d->targets + r0;
        a.rows = n;
        a.term = term + r0;
        a.dx = (unsigned char *)dx + (size_t)r0 * g.K * elem;
        if ((rc = step_launch_k<true>(g.bf16, g.K, a, stream))) return rc;
        if ((rc = launch_product_tn(g.bf16 ? MOT_BF16 : MOT_F32, a.G, kV, kV, g.bf16 ? a.x : a.aux, g.K, g.K, n, dW, g.K, stream))) return rc;
    }
    return launch_head_loss(term, g.rows, (double *)(ws + w.part), 1.0 / (double)g.rows, d->loss, stream);
}

}  // namespace mot
