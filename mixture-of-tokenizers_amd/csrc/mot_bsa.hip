// mot_bsa.hip -- byte self-attention of the concat mixin (ByteSelfAttn around CausalSelfAttention,
// scaled-pre-train/train_gpt.py:382-418, 209-240): out = x + c_proj(attn(qkv(x))), forward and backward, fp32.
//
// The attention is banded: query i of a batch row sees key j when i - j < W (W <= 256 bytes) and j <= i (causal) or
// j / bpt <= i / bpt (block-causal).  A workgroup owns 128 consecutive positions of one (batch row, head), a wave 32 of them, and
// walks the few 32-position chunks of the other side that the band reaches; there is no loop over the sequence.
//
// Products run on v_mfma_f32_32x32x2_f32, TRANSPOSED: the score block is S^T[key][query] = K Q^T, so that in the accumulator
// layout (column = lane & 31, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) a lane holds ONE query and 16 of the chunk's keys.  The
// softmax statistics of a query are then lane-local (plus one exchange with lane ^ 32), and the 16 registers are, as they stand,
// the B operand of the second product O^T[col][query] += V^T[col][key] P^T[key][query] -- the reduction index of an MFMA may be
// taken in any order as long as both operands agree, and step r takes keys {row(r, 0), row(r, 1)}.  Nothing is transposed through LDS.
// The first product takes the 128 head columns in the order (lane >> 5) * 64 + s, so its LDS operand is read 16 bytes at a time.
//
// No running maximum: q and k are rms-normalised per head (sum of squares <= 128, rotary keeps it), so |0.12 q.k| <= 15.36 and
// exp of it lies in [2e-7, 5e6]; a window of 256 + 63 such terms neither overflows nor underflows fp32.  The kernels take
// p = exp2(s) with 0.12 log2(e) folded into q, keep sum p, and save log2(sum p) per (row, head); the backward recomputes p from it.
//
// Backward, two passes with the same tiling and no atomics: one walks query tiles (dq), one walks key tiles (dk, dv, and the
// per-workgroup partial of d lambda, summed afterwards in a fixed order).  Both end by taking their accumulators back through the
// rotary step and the norm inside the kernel, and write the gradient of the raw projections.
// The projections (x qkv_w^T, y c_proj^T, and their backward products) go through the shared launchers of mot_internal.hpp.
#include <float.h>

#include "mot_internal.hpp"

namespace mot {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBsaThreads = 256;   // 4 waves, 32 positions each
constexpr int kTile = 128;         // positions per workgroup
constexpr int kChunk = 32;         // positions of the other side per step
constexpr int kLd = 132;           // LDS row stride in floats: 16-byte rows, b128 reads of 16 consecutive rows touch every bank once
constexpr float kAttnScale = 0.12f;                       // CausalSelfAttention.attn_scale
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;
constexpr float kQScale = kAttnScale * kLog2e;

__device__ __forceinline__ float xor_add(float v, int m) { return v + __shfl_xor(v, m, 64); }

// 32 rows [row0, row0 + 32) of one head's q or k (128 floats at src + pos * ld) -> rms-norm, rotary, * scale -> dst[32][kLd].
// 8 threads a row: thread t takes columns 8t .. 8t+7 and 64+8t .. 64+8t+7 (the two rotary partners).  Rows outside [0, L) are zeros.
__device__ __forceinline__ void stage_rope(float *__restrict__ dst, const float *__restrict__ src, int64_t ld, int row0, int L,
                                           const float *__restrict__ cosT, const float *__restrict__ sinT, float eps, float scale) {
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7, pos = row0 + row;
    f32x4 a[2], b[2], c[2], s[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) { a[e] = (f32x4)(0.f); b[e] = (f32x4)(0.f); c[e] = (f32x4)(1.f); s[e] = (f32x4)(0.f); }
    if (pos < L) {
        const float *p = src + (int64_t)pos * ld + 8 * t;
        const float *pc = cosT + (int64_t)pos * 64 + 8 * t, *ps = sinT + (int64_t)pos * 64 + 8 * t;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            a[e] = *(const f32x4 *)(p + 4 * e);
            b[e] = *(const f32x4 *)(p + 64 + 4 * e);
            c[e] = *(const f32x4 *)(pc + 4 * e);
            s[e] = *(const f32x4 *)(ps + 4 * e);
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
        for (int q = 0; q < 4; ++q) ss += a[e][q] * a[e][q] + b[e][q] * b[e][q];
    ss = xor_add(ss, 1); ss = xor_add(ss, 2); ss = xor_add(ss, 4);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / 128.0f) + eps);
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const f32x4 x1 = a[e] * rstd, x2 = b[e] * rstd;
        const f32x4 y1 = x1 * c[e] + x2 * s[e], y2 = x2 * c[e] - x1 * s[e];
        *(f32x4 *)(dst + row * kLd + 8 * t + 4 * e) = y1 * scale;
        *(f32x4 *)(dst + row * kLd + 64 + 8 * t + 4 * e) = y2 * scale;
    }
}

// the same rows of v or dy, * scale, no norm
__device__ __forceinline__ void stage_plain(float *__restrict__ dst, const float *__restrict__ src, int64_t ld, int row0, int L, float scale) {
    const int row = threadIdx.x >> 3, t = threadIdx.x & 7, pos = row0 + row;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int col = (e & 1) * 4 + (e >> 1) * 64 + 8 * t;
        f32x4 v = (f32x4)(0.f);
        if (pos < L) v = *(const f32x4 *)(src + (int64_t)pos * ld + col);
        *(f32x4 *)(dst + row * kLd + col) = v * scale;
    }
}

// S^T block: sum over the 128 columns of lds[lane & 31][col] (A operand) * frag[col] (B operand: the wave's own 32 rows)
__device__ __forceinline__ f32x16 dot128(const float *__restrict__ lds, const float (&frag)[64], int li, int h) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const float *p = lds + li * kLd + 64 * h;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const f32x4 a = *(const f32x4 *)(p + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], frag[4 * c + e], s, 0, 0, 0);
    }
    return s;
}

// acc[nb][.] += sum over the chunk's 32 rows of lds[row][32 nb + lane & 31] * w[row]   (w in accumulator layout: register r = row(r, h))
__device__ __forceinline__ void accum_rows(f32x16 (&acc)[4], const float *__restrict__ lds, const f32x16 &w, int li, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float *p = lds + ((r & 3) + 8 * (r >> 2) + 4 * h) * kLd + li;
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[32 * nb], w[r], acc[nb], 0, 0, 0);
    }
}

// a wave's 32 rows of the staged block as the B operand of dot128: frag[s] = lds[lane & 31][64 (lane >> 5) + s]
__device__ __forceinline__ void read_frag(float (&frag)[64], const float *__restrict__ lds, int li, int h) {
    const float *p = lds + li * kLd + 64 * h;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        const f32x4 v = *(const f32x4 *)(p + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) frag[4 * c + e] = v[e];
    }
}

// the same operand straight from global memory (rows that need no norm), * scale
__device__ __forceinline__ void load_frag(float (&frag)[64], const float *__restrict__ row, bool valid, float scale, int h) {
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        f32x4 v = (f32x4)(0.f);
        if (valid) v = *(const f32x4 *)(row + 64 * h + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) frag[4 * c + e] = v[e] * scale;
    }
}

// Gradient of one position's q or k from the gradient of its normalised, rotated row.  acc[nb][4g + e] belongs to column
// 32 nb + 8 g + 4 h + e of position `pos` (lane & 31); the rotary partner of a column of block nb < 2 is the same register of block
// nb + 2.  With y = x rstd:  dy = R^T acc * scale,  dx = rstd (dy - y (dy . y) / 128).  `raw` is the projected row as the forward saw it.
__device__ __forceinline__ void rope_norm_bwd(const f32x16 (&acc)[4], const float *__restrict__ raw, float *__restrict__ out, bool valid, int pos,
                                              const float *__restrict__ cosT, const float *__restrict__ sinT, float eps, float scale, int h) {
    f32x4 x[4][4];
    float ss = 0.f;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            x[nb][g] = (f32x4)(0.f);
            if (valid) x[nb][g] = *(const f32x4 *)(raw + 32 * nb + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) ss += x[nb][g][e] * x[nb][g][e];
        }
    ss = xor_add(ss, 32);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / 128.0f) + eps);
    f32x4 d[4][4];
    float dot = 0.f;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 c = (f32x4)(1.f), s = (f32x4)(0.f);
            if (valid) {
                c = *(const f32x4 *)(cosT + (int64_t)pos * 64 + 32 * nb + 8 * g + 4 * h);
                s = *(const f32x4 *)(sinT + (int64_t)pos * 64 + 32 * nb + 8 * g + 4 * h);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float g1 = acc[nb][4 * g + e] * scale, g2 = acc[nb + 2][4 * g + e] * scale;
                d[nb][g][e] = g1 * c[e] - g2 * s[e];
                d[nb + 2][g][e] = g1 * s[e] + g2 * c[e];
                dot += d[nb][g][e] * (x[nb][g][e] * rstd) + d[nb + 2][g][e] * (x[nb + 2][g][e] * rstd);
            }
        }
    dot = xor_add(dot, 32) * (1.0f / 128.0f);
    if (valid)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb)
#pragma unroll
            for (int g = 0; g < 4; ++g) *(f32x4 *)(out + 32 * nb + 8 * g + 4 * h) = (d[nb][g] - x[nb][g] * rstd * dot) * rstd;
}

struct BsaArgs {
    const float *qkv;     // [B L][3 H 128] raw projections
    const float *cosT, *sinT, *lambda;
    float *y;             // [B L][H 128]  (forward: written; backward: read)
    float *lse;           // [B][H][L] log2 of the row sums
    const float *dy;      // backward: [B L][H 128]
    float *dqkv;          // backward: [B L][3 H 128]
    float *partial;       // backward: one d lambda partial per workgroup of the key pass
    int L, H, bpt, W, bc;
    float eps;
};

// last key a query sees / first query that sees a key
__device__ __forceinline__ int last_key(int i, int bpt, int bc) { return bc ? (i / bpt + 1) * bpt - 1 : i; }
__device__ __forceinline__ int first_query(int j, int bpt, int bc) { return bc ? (j / bpt) * bpt : j; }

// BWD = false: forward (y, lse).  BWD = true: backward over query tiles (dq).
template <bool BWD>
__global__ __launch_bounds__(kBsaThreads, BWD ? 1 : 2) void bsa_query_kernel(BsaArgs a) {
    __shared__ __attribute__((aligned(16))) float sK[kChunk * kLd], sV[kChunk * kLd];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, li = lane & 31;
    const int L = a.L, hd = blockIdx.y, HD = a.H * 128;
    const int64_t ld = 3 * (int64_t)HD, row_base = (int64_t)blockIdx.z * L;
    const int q0 = blockIdx.x * kTile, qlo = q0 + wave * 32, i = qlo + li;
    const bool valid = i < L;
    const float *qp = a.qkv + row_base * ld + hd * 128, *kp = qp + HD, *vp = qp + 2 * HD;
    const float lam = *a.lambda;

    float qf[64];
    for (int w = 0; w < 4; ++w) {
        stage_rope(sK, qp, ld, q0 + 32 * w, L, a.cosT, a.sinT, a.eps, kQScale);
        __syncthreads();
        if (w == wave) read_frag(qf, sK, li, h);
        __syncthreads();
    }
    float df[64];
    float lse_i = 0.f, delta_i = 0.f;
    if (BWD) {
        const float *dyr = a.dy + (row_base + i) * HD + hd * 128, *yr = a.y + (row_base + i) * HD + hd * 128;
        load_frag(df, dyr, valid, 1.0f, h);
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            f32x4 v = (f32x4)(0.f);
            if (valid) v = *(const f32x4 *)(yr + 64 * h + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) delta_i += v[e] * df[4 * c + e];
        }
        delta_i = xor_add(delta_i, 32);
        if (valid) lse_i = a.lse[((int64_t)blockIdx.z * a.H + hd) * L + i];
    }

    f32x16 acc[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
    float lsum = 0.f;

    const int jmin = i - a.W + 1, jmax = last_key(i, a.bpt, a.bc);
    const int wlo = qlo - a.W + 1, whi = last_key(qlo + 31, a.bpt, a.bc);            // keys this wave's queries can see
    int kstart = q0 - a.W + 1;
    kstart = kstart < 0 ? 0 : kstart & ~(kChunk - 1);
    int kend = last_key(q0 + kTile - 1, a.bpt, a.bc) + 1;
    kend = kend > L ? L : kend;
    for (int kc = kstart; kc < kend; kc += kChunk) {
        stage_rope(sK, kp, ld, kc, L, a.cosT, a.sinT, a.eps, 1.0f);
        stage_plain(sV, vp, ld, kc, L, lam);
        __syncthreads();
        if (qlo < L && kc + kChunk - 1 >= wlo && kc <= whi) {
            f32x16 s = dot128(sK, qf, li, h);
            f32x16 w;
            if (!BWD) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = kc + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const bool ok = valid && j >= jmin && j <= jmax && j < L;
                    w[r] = ok ? __builtin_amdgcn_exp2f(s[r]) : 0.f;
                    lsum += w[r];
                }
                accum_rows(acc, sV, w, li, h);
            } else {
                const f32x16 dp = dot128(sV, df, li, h);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int j = kc + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const bool ok = valid && j >= jmin && j <= jmax && j < L;
                    const float p = ok ? __builtin_amdgcn_exp2f(s[r] - lse_i) : 0.f;
                    w[r] = p * (dp[r] - delta_i);
                }
                accum_rows(acc, sK, w, li, h);
            }
        }
        __syncthreads();
    }

    if (!BWD) {
        lsum = xor_add(lsum, 32);
        if (valid) {
            const float inv = 1.0f / lsum;
            float *yr = a.y + (row_base + i) * HD + hd * 128;
#pragma unroll
            for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[nb][4 * g + e] * inv;
                    *(f32x4 *)(yr + 32 * nb + 8 * g + 4 * h) = v;
                }
            if (h == 0) a.lse[((int64_t)blockIdx.z * a.H + hd) * L + i] = log2f(lsum);
        }
    } else {
        const int64_t off = (row_base + i) * ld + hd * 128;
        rope_norm_bwd(acc, a.qkv + off, a.dqkv + off, valid, i, a.cosT, a.sinT, a.eps, kAttnScale, h);
    }
}

// backward over key tiles: dk, dv and the workgroup's share of d lambda
__global__ __launch_bounds__(kBsaThreads) void bsa_key_kernel(BsaArgs a) {
    __shared__ __attribute__((aligned(16))) float sQ[kChunk * kLd], sD[kChunk * kLd];
    __shared__ float sLse[kChunk], sDelta[kChunk], sRed[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, h = lane >> 5, li = lane & 31;
    const int L = a.L, hd = blockIdx.y, HD = a.H * 128;
    const int64_t ld = 3 * (int64_t)HD, row_base = (int64_t)blockIdx.z * L;
    const int j0 = blockIdx.x * kTile, jlo = j0 + wave * 32, j = jlo + li;
    const bool valid = j < L;
    const float *qp = a.qkv + row_base * ld + hd * 128, *kp = qp + HD, *vp = qp + 2 * HD;
    const float *dyp = a.dy + row_base * HD + hd * 128, *yp = a.y + row_base * HD + hd * 128;
    const float *lsep = a.lse + ((int64_t)blockIdx.z * a.H + hd) * L;
    const float lam = *a.lambda;

    float kf[64], vf[64];
    for (int w = 0; w < 4; ++w) {
        stage_rope(sQ, kp, ld, j0 + 32 * w, L, a.cosT, a.sinT, a.eps, 1.0f);
        __syncthreads();
        if (w == wave) read_frag(kf, sQ, li, h);
        __syncthreads();
    }
    load_frag(vf, vp + (int64_t)j * ld, valid, lam, h);

    f32x16 dk[4], dv[4];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dk[nb][r] = 0.f; dv[nb][r] = 0.f; }

    const int imin = first_query(j, a.bpt, a.bc), imax = j + a.W - 1;
    const int wlo = first_query(jlo, a.bpt, a.bc), whi = jlo + 31 + a.W - 1;           // queries that can see this wave's keys
    const int qstart = first_query(j0, a.bpt, a.bc) & ~(kChunk - 1);
    int qend = j0 + kTile - 1 + a.W;
    qend = qend > L ? L : qend;
    for (int qc = qstart; qc < qend; qc += kChunk) {
        stage_rope(sQ, qp, ld, qc, L, a.cosT, a.sinT, a.eps, kQScale);
        stage_plain(sD, dyp, HD, qc, L, 1.0f);
        {   // delta = dy . y and lse of the chunk's rows: the 8 threads of a row, as in the staging
            const int row = threadIdx.x >> 3, t = threadIdx.x & 7, pos = qc + row;
            float d = 0.f;
            if (pos < L)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int col = (e & 1) * 4 + (e >> 1) * 64 + 8 * t;
                    const f32x4 u = *(const f32x4 *)(dyp + (int64_t)pos * HD + col), v = *(const f32x4 *)(yp + (int64_t)pos * HD + col);
#pragma unroll
                    for (int q = 0; q < 4; ++q) d += u[q] * v[q];
                }
            d = xor_add(d, 1); d = xor_add(d, 2); d = xor_add(d, 4);
            if (t == 0) { sDelta[row] = d; sLse[row] = pos < L ? lsep[pos] : 0.f; }
        }
        __syncthreads();
        if (jlo < L && qc + kChunk - 1 >= wlo && qc <= whi) {
            const f32x16 s = dot128(sQ, kf, li, h);
            const f32x16 dp = dot128(sD, vf, li, h);
            f32x16 p, ds;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h, i = qc + row;
                const bool ok = valid && i >= imin && i <= imax && i < L;
                p[r] = ok ? __builtin_amdgcn_exp2f(s[r] - sLse[row]) : 0.f;
                ds[r] = p[r] * (dp[r] - sDelta[row]);
            }
            accum_rows(dv, sD, p, li, h);
            accum_rows(dk, sQ, ds, li, h);
        }
        __syncthreads();
    }

    const int64_t off = (row_base + j) * ld + hd * 128;
    // sQ holds 0.12 log2(e) q: the log2(e) comes out here
    rope_norm_bwd(dk, a.qkv + off + HD, a.dqkv + off + HD, valid, j, a.cosT, a.sinT, a.eps, kLn2, h);
    float dl = 0.f;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v = (f32x4)(0.f), o;
            if (valid) v = *(const f32x4 *)(a.qkv + off + 2 * HD + 32 * nb + 8 * g + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) { dl += dv[nb][4 * g + e] * v[e]; o[e] = dv[nb][4 * g + e] * lam; }
            if (valid) *(f32x4 *)(a.dqkv + off + 2 * HD + 32 * nb + 8 * g + 4 * h) = o;
        }
    dl = xor_add(dl, 32); dl = xor_add(dl, 16); dl = xor_add(dl, 8); dl = xor_add(dl, 4); dl = xor_add(dl, 2); dl = xor_add(dl, 1);
    if (lane == 0) sRed[wave] = dl;
    __syncthreads();
    if (threadIdx.x == 0)
        a.partial[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// d lambda = sum of the partials, in a fixed order (one workgroup)
__global__ __launch_bounds__(kBsaThreads) void bsa_sum_partials_kernel(const float *__restrict__ partial, int64_t n, float *__restrict__ out) {
    __shared__ float red[kBsaThreads];
    float v = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += kBsaThreads) v += partial[i];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBsaThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// dst = src (a kernel, not a memcpy node, so that the call sequence replays from a captured graph)
__global__ __launch_bounds__(kBsaThreads) void bsa_copy_kernel(const float *__restrict__ src, float *__restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kBsaThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBsaThreads) dst[i] = src[i];
}

int copy_floats(const float *src, float *dst, int64_t n, hipStream_t stream) {
    int64_t blocks = (n + kBsaThreads - 1) / kBsaThreads;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(bsa_copy_kernel, dim3((unsigned)blocks), dim3(kBsaThreads), 0, stream, src, dst, n);
    return check_launch("bsa_copy_kernel");
}

struct Saved {
    float *qkv, *y, *lse;
};
Saved saved_of(const MotByteSelfAttnDesc &d) {
    const int64_t n = d.n_rows * d.row_len, HD = (int64_t)d.n_heads * 128;
    float *p = (float *)d.saved;
    return {p, p + n * 3 * HD, p + n * 4 * HD};
}

BsaArgs args_of(const MotByteSelfAttnDesc &d, const Saved &s) {
    BsaArgs a{};
    a.qkv = s.qkv; a.y = s.y; a.lse = s.lse;
    a.cosT = d.cos; a.sinT = d.sin; a.lambda = d.lambda_v;
    a.L = (int)d.row_len; a.H = d.n_heads; a.bpt = d.bpt; a.W = d.window; a.bc = d.block_causal ? 1 : 0;
    a.eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    return a;
}

dim3 grid_of(const MotByteSelfAttnDesc &d) {
    return dim3((unsigned)((d.row_len + kTile - 1) / kTile), (unsigned)d.n_heads, (unsigned)d.n_rows);
}

}  // namespace

size_t byte_self_attn_saved_bytes(const MotByteSelfAttnDesc &d) {
    const int64_t n = d.n_rows * d.row_len, HD = (int64_t)d.n_heads * 128;
    return (size_t)(n * 4 * HD + n * d.n_heads) * sizeof(float);
}

// the backward's dy [n, HD], d qkv [n, 3 HD] and the d lambda partials; the forward needs none of it
size_t byte_self_attn_workspace_bytes(const MotByteSelfAttnDesc &d) {
    const int64_t n = d.n_rows * d.row_len, HD = (int64_t)d.n_heads * 128;
    const int64_t blocks = (d.row_len + kTile - 1) / kTile * d.n_heads * d.n_rows;
    return (size_t)(n * 4 * HD + (blocks + 3) / 4 * 4) * sizeof(float);
}

int launch_byte_self_attn_fwd(const MotByteSelfAttnDesc &d, hipStream_t stream) {
    const int64_t n = d.n_rows * d.row_len;
    const int D = d.dim, HD = d.n_heads * 128;
    const Saved s = saved_of(d);
    if (int rc = launch_gemm_rows((const float *)d.x, D, n, (const float *)d.qkv_w, D, D, 3 * HD, s.qkv, 3 * HD, true, stream)) return rc;
    const BsaArgs a = args_of(d, s);
    hipLaunchKernelGGL(bsa_query_kernel<false>, grid_of(d), dim3(kBsaThreads), 0, stream, a);
    if (int rc = check_launch("bsa_query_kernel<fwd>")) return rc;
    if (int rc = copy_floats((const float *)d.x, (float *)d.out, n * D, stream)) return rc;
    return launch_gemm_rows(s.y, HD, n, (const float *)d.proj_w, HD, HD, D, (float *)d.out, D, true, stream, nullptr, true);
}

int launch_byte_self_attn_bwd(const MotByteSelfAttnDesc &d, const MotByteSelfAttnGrads &g, hipStream_t stream) {
    const int64_t n = d.n_rows * d.row_len;
    const int D = d.dim, HD = d.n_heads * 128;
    const Saved s = saved_of(d);
    float *dy = (float *)d.workspace, *dqkv = dy + n * HD, *partial = dqkv + n * 3 * HD;
    const float *go = (const float *)g.grad_out;
    // dy = g c_proj  (c_proj.weight is [D, HD]: the natural layout of the B operand)
    if (int rc = launch_gemm_rows(go, D, n, (const float *)d.proj_w, HD, D, HD, dy, HD, false, stream)) return rc;
    if (g.d_proj_w) {
        if (int rc = launch_zero_words(g.d_proj_w, (int64_t)D * HD, stream)) return rc;
        if (int rc = launch_gemm_tn(go, D, D, s.y, HD, HD, n, (float *)g.d_proj_w, HD, stream)) return rc;
    }
    BsaArgs a = args_of(d, s);
    a.dy = dy; a.dqkv = dqkv; a.partial = partial;
    const dim3 grid = grid_of(d);
    hipLaunchKernelGGL(bsa_query_kernel<true>, grid, dim3(kBsaThreads), 0, stream, a);
    if (int rc = check_launch("bsa_query_kernel<bwd>")) return rc;
    hipLaunchKernelGGL(bsa_key_kernel, grid, dim3(kBsaThreads), 0, stream, a);
    if (int rc = check_launch("bsa_key_kernel")) return rc;
    if (g.d_lambda) {
        hipLaunchKernelGGL(bsa_sum_partials_kernel, dim3(1), dim3(kBsaThreads), 0, stream, (const float *)partial, (int64_t)grid.x * grid.y * grid.z, g.d_lambda);
        if (int rc = check_launch("bsa_sum_partials_kernel")) return rc;
    }
    if (g.d_qkv_w) {
        if (int rc = launch_zero_words(g.d_qkv_w, (int64_t)3 * HD * D, stream)) return rc;
        if (int rc = launch_gemm_tn(dqkv, 3 * HD, 3 * HD, (const float *)d.x, D, D, n, (float *)g.d_qkv_w, D, stream)) return rc;
    }
    if (g.dx) {
        if (int rc = copy_floats(go, (float *)g.dx, n * D, stream)) return rc;
        // dx = g + dqkv qkv_w  (qkv_w flattened is [3 HD, D])
        if (int rc = launch_gemm_rows(dqkv, 3 * HD, n, (const float *)d.qkv_w, D, 3 * HD, D, (float *)g.dx, D, false, stream, nullptr, true)) return rc;
    }
    return MOT_OK;
}

}  // namespace mot
