// mot_once.hip -- the write-once backward of the fused front-end (include/mot.h, MotEmbedMixGradsOnce):
// MOT_MIX_SUM, MOT_MIX_NOOP and MOT_MIX_CONCAT with one id tensor, fp32 and bf16.  The token-table gradient is written once, in the
// table's dtype, as fp32 sums in ascending position order with +0 rows for absent ids: no atomic touches a gradient element, the
// caller zeroes nothing, and every run gives the same bits.  No piece of the workspace is proportional to N x D: d a_n is FORMED
// in token order by the kernel that sums it, from grad_out, the tables and four fp32 scalars per position.
//
// With a^ = r_t a (norm_tok, else a), b^_k = r_k b_k (norm_byte, else b_k), y = s_t a^ (+) s_b b^ per the mode, x = r_o y (norm_out):
//     dy   = r_o (g - x c_o),  c_o = (g . x) / D            (norm_out; else dy = g)
//     d a  = r_t (s_t dy - a^ c_t),  c_t = (s_t dy . a^) / Dt   (norm_tok; else d a = s_t dy), over the token columns
//     d b_k = r_k (s_b dy_k - b^_k (s_b dy_k . b^_k) / Db)       (norm_byte; else s_b dy_k), over slot k's columns
//     d s_t = sum_n dy . a^,  d s_b = sum_n dy . b^
//
//   once_rows_kernel <T, NCH>      pass A, position order: a wave per position, four positions one after the other, NCH 16-byte
//                                  chunks per lane.  Recomputes the forward row in fp32 from the tables (nothing is re-rounded),
//                                  writes {r_o, c_o, r_t, c_t} per position (16 bytes), the fp32 d b rows of a slab of 16 384
//                                  positions with the slab's largest |element|, and one pair of scale-gradient partials per 16
//                                  positions.
//   once_byte_sums_kernel,         the slab's d b rows summed into the byte table in 64-bit fixed point (integer LDS and global
//   once_byte_close_kernel         atomics: the sums do not depend on the order of the adds), converted and added to d_byte slab by
//                                  slab.  (The LDS sums of mot_bytecat.hip flush with float atomics: not the same bits on every run.)
//   once_scalars_kernel            ONE workgroup adds the partials in order.
//   once_slices_kernel <T, BYTES>  pass B, token order: the partition of ve_bwd_slices_kernel (mot_values.hip) -- a wave owns a slice
//                                  of 64 sorted slots and 64 16-byte chunks of columns, eight rows in flight -- but every row is
//                                  formed: g[p][cols], the position's scalars, the group's token-row piece (one address per group:
//                                  HBM sees it once, the later requests hit L1 / L2; keeping it in registers across the rows in
//                                  flight cost 234 VGPRs + 96 AGPRs in fp32, one wave per SIMD) and, where the forward has a byte part in the token
//                                  columns and an output norm (BYTES: SUM with norm_out), the byte-row piece via ids[p, slot].
//                                  Groups inside the slice are rounded and stored once (non-temporal); head and tail pieces go
//                                  to the workspace in fp32, and ve_bwd_rows_kernel (unchanged) closes: pieces in ascending slice
//                                  order in four fixed quarters, +0 rows.
//
// Resources of every instantiation, from the compiler's own remarks (-Rpass-analysis=kernel-resource-usage, gfx950:
// VGPRs (+ AGPRs) / SGPRs / scratch bytes per lane / static LDS bytes / waves per SIMD):
//   once_rows_kernel   <bf16, 1>   76 / 103 / 0 / 9248 / 6     <bf16, 2>  131 / 106 / 0 / 9248 / 3     <bf16, 4>  214 / 106 / 0 / 9248 / 2
//                      <fp32, 1>   58 /  95 / 0 / 9248 / 8     <fp32, 4>  157 / 106 / 0 / 9248 / 3     <fp32, 8>  256 + 42 / 106 / 0 / 9248 / 1
//   once_slices_kernel <bf16, no bytes>  122 / 58 / 0 / 0 / 4     <bf16, bytes>  170 / 68 / 0 / 0 / 2
//                      <fp32, no bytes>  106 / 54 / 0 / 0 / 4     <fp32, bytes>  148 / 64 / 0 / 0 / 3
//   once_scalars_kernel  34 / 18 / 0 / 2048 / 8     once_byte_sums_kernel  44 / 52 / 0 / dynamic, <= 64 KiB / 8     once_byte_close_kernel  12 / 14 / 0 / 0 / 8
// No instantiation uses scratch.  <fp32, 8> of the row kernel (fp32 rows above 1024 columns) keeps three rows of eight chunks in
// registers and runs one wave per SIMD; the headline shapes take <fp32, 4> and <bf16, 2>.
#include "mot_wave.hpp"

namespace mot {

constexpr int kOnceMaxDim = 2048;
constexpr int64_t kOnceSlab = 16384;            // positions per slab of the byte part's fp32 rows: 48 MiB at 768 columns
constexpr int kOnceTok = 4;                     // positions per wave of the row kernel
constexpr int kOnceBlockTok = kOnceTok * kWaves;   // positions per workgroup: one pair of scalar partials each
constexpr int kOnceOrderLimit = (1 << 21) - 1;  // the token order's limit on the table height (mot_group.hip)
constexpr int kOnceByteChunk = 512;             // positions per workgroup of the byte table's sums
constexpr int kOnceSlice = 64;                  // sorted slots per wave of the slices kernel (kVeSlice, mot_values.hip)

// ------------------------------------------------------------------------------------------ pass A
struct OnceRowsArgs {
    const int32_t *tokens;      // the launch's first position
    const int64_t *ids;         // likewise; null for NOOP
    const void *tok_table, *byte_table;
    const float *byte_rnorm;    // the byte rows' rms factors, or null (no norm_byte)
    const void *g;              // the launch's first row of grad_out
    const float *s_t, *s_b;     // device scalars or null (= 1)
    float4v *scal;              // [n] {r_o, c_o, r_t, c_t}
    float *dub;                 // [n][bpt * Db] fp32 or null
    float *part;                // [blocks][2] of this launch, or null
    uint32_t *gmax;             // the bits of the largest finite |d b| element of this launch (with dub)
    int64_t n;
    int tok_rows, byte_rows, bpt, Db, Dt, D;
    int mode, norm_tok, norm_out;
    float eps;
    uint32_t *status;
};

// NCH: 16-byte chunks per lane (covers D <= 64 * NCH * VEC).
template <typename T, int NCH>
__global__ __launch_bounds__(kThreads) void once_rows_kernel(const OnceRowsArgs A) {
    typedef typename Elem<T>::vec vec_t;
    constexpr int VEC = Elem<T>::kVec;
    __shared__ float parts[kWaves][kOnceMaxDim / 4];   // a chunk's share of its slot's dot
    __shared__ float dots[kWaves][kMaxBpt];
    __shared__ float red[kWaves][2];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = A.D, Dt = A.Dt, Db = A.Db, bpt = A.bpt, nv = D / VEC;
    const bool bytes = A.mode != MOT_MIX_NOOP;
    const int byte_lo = A.mode == MOT_MIX_CONCAT ? Dt : 0;   // the column where the byte part begins
    const int nbk = bpt * Db, L = bytes ? Db / VEC : 1, c_lo = byte_lo / VEC;
    const T *tok_table = (const T *)A.tok_table, *byte_table = (const T *)A.byte_table;
    const T *g = (const T *)A.g;
    const float s_t = A.s_t ? *A.s_t : 1.f, s_b = A.s_b ? *A.s_b : 1.f;
    const float inv_D = 1.0f / (float)D, inv_Dt = 1.0f / (float)Dt, inv_Db = 1.0f / (float)(bytes ? Db : 1);
    // column VEC * j of a row: a token column when below Dt, a column of byte slot kk (at `within` of its row) when at or above byte_lo
    bool tcol[NCH], bcol[NCH];
    int kk[NCH], within[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int j = lane + 64 * i, col = VEC * j;
        tcol[i] = j < nv && col < Dt;
        bcol[i] = bytes && j < nv && col >= byte_lo;
        const int cb = bcol[i] ? col - byte_lo : 0;
        kk[i] = cb / (bytes ? Db : 1);
        within[i] = cb - kk[i] * Db;
    }
    float acc_t = 0.f, acc_b = 0.f;   // the lane's share of d s_t and d s_b over the wave's positions
    float mx = 0.f;                   // the lane's largest finite |d b| element over the wave's positions
    const int64_t n0 = ((int64_t)blockIdx.x * kWaves + wave) * kOnceTok;
    for (int q = 0; q < kOnceTok; ++q) {
        const int64_t n = n0 + q;
        if (n >= A.n) break;   // wave-uniform; the barrier is behind the loop
        int tok = A.tokens[n];
        if ((uint64_t)(uint32_t)tok >= (uint64_t)A.tok_rows) {
            if (A.status && lane == 0) atomicOr(A.status, kStatusTokenOor);
            tok = 0;
        }
        const T *arow = tok_table + (int64_t)tok * Dt;
        vec_t a[NCH], b[NCH], h[NCH];
        float rk[NCH];
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int j = lane + 64 * i;
            a[i] = (vec_t)(0.f); b[i] = (vec_t)(0.f); h[i] = (vec_t)(0.f); rk[i] = 1.f;
            if (j < nv) h[i] = Elem<T>::loadv(g + n * D + VEC * j);
            if (tcol[i]) {
                a[i] = Elem<T>::loadv(arow + VEC * j);
#pragma unroll
                for (int e = 0; e < VEC; ++e) ss += a[i][e] * a[i][e];
            }
            if (bcol[i]) {
                int64_t id = A.ids[n * bpt + kk[i]];
                if ((uint64_t)id >= (uint64_t)A.byte_rows) { if (A.status) atomicOr(A.status, kStatusByteOor); id = 0; }
                if (A.byte_rnorm) rk[i] = A.byte_rnorm[id];
                b[i] = Elem<T>::loadv(byte_table + id * Db + within[i]) * rk[i];   // b^
            }
        }
        float r_t = 1.f, r_o = 1.f, c_o = 0.f, c_t = 0.f;
        if (A.norm_tok) {
            r_t = rms_scale(wave_sum(ss), Dt, A.eps);
#pragma unroll
            for (int i = 0; i < NCH; ++i) a[i] *= r_t;   // a^
        }
        if (A.norm_out) {
            float sy = 0.f, gy = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const vec_t y = a[i] * s_t + b[i] * s_b;
#pragma unroll
                for (int e = 0; e < VEC; ++e) { sy += y[e] * y[e]; gy += h[i][e] * y[e]; }
            }
            r_o = rms_scale(wave_sum(sy), D, A.eps);
            c_o = wave_sum(gy) * r_o * inv_D;
            const float f = r_o * c_o;
#pragma unroll
            for (int i = 0; i < NCH; ++i) h[i] = (h[i] - (a[i] * s_t + b[i] * s_b) * f) * r_o;   // dy
        }
        float da = 0.f, db = 0.f;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            float p = 0.f, u = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) { p += h[i][e] * a[i][e]; u += h[i][e] * b[i][e]; }
            da += p;   // (a and b are zero outside their columns)
            db += u;
            if (bcol[i]) parts[wave][lane + 64 * i - c_lo] = u * s_b;
        }
        acc_t += da;
        acc_b += db;
        if (A.norm_tok) c_t = wave_sum(da) * s_t * inv_Dt;
        if (lane == 0) A.scal[n] = float4v{r_o, c_o, r_t, c_t};
        if (A.dub) {
            if (A.byte_rnorm) {
                wave_lds_sync();
                if (lane < bpt) {   // one lane per slot: its L chunks in chunk order
                    float s = 0.f;
                    for (int c = 0; c < L; ++c) s += parts[wave][lane * L + c];
                    dots[wave][lane] = s * inv_Db;
                }
                wave_lds_sync();
            }
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                if (!bcol[i]) continue;
                vec_t du = h[i] * s_b;
                if (A.byte_rnorm) du = (du - b[i] * dots[wave][kk[i]]) * rk[i];
                *(vec_t *)(A.dub + n * nbk + kk[i] * Db + within[i]) = du;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    const float av = fabsf(du[e]);
                    if (av < INFINITY) mx = fmaxf(mx, av);
                }
            }
            if (A.byte_rnorm) wave_lds_sync();   // the next position overwrites parts
        }
    }
    if (A.dub) {   // a maximum is the same whatever the order; the atomic only where it would raise the word (same-address atomics serialise)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (lane == 0 && mx > 0.f && __float_as_uint(mx) > __hip_atomic_load(A.gmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(A.gmax, __float_as_uint(mx));
    }
    if (!A.part) return;   // uniform over the workgroup
    const float st = wave_sum(acc_t), sb = wave_sum(acc_b);
    if (lane == 0) { red[wave][0] = st; red[wave][1] = sb; }
    __syncthreads();
    if (threadIdx.x == 0) {   // the four waves in wave order
        A.part[2 * (int64_t)blockIdx.x] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        A.part[2 * (int64_t)blockIdx.x + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
}

constexpr int kOnceSumThreads = 256;
__global__ __launch_bounds__(kOnceSumThreads) void once_scalars_kernel(const float *__restrict__ part, int64_t nblk, float *__restrict__ ds_t,
                                                                       float *__restrict__ ds_b) {
    __shared__ float s[kOnceSumThreads][2];
    const int tid = threadIdx.x;
    const int64_t per = (nblk + kOnceSumThreads - 1) / kOnceSumThreads;
    const int64_t lo = min(nblk, tid * per), hi = min(nblk, lo + per);
    float a = 0.f, b = 0.f;
    for (int64_t i = lo; i < hi; ++i) { a += part[2 * i]; b += part[2 * i + 1]; }
    s[tid][0] = a; s[tid][1] = b;
    __syncthreads();
    if (tid == 0) {
        a = 0.f; b = 0.f;
        for (int i = 0; i < kOnceSumThreads; ++i) { a += s[i][0]; b += s[i][1]; }
        if (ds_t) *ds_t = a;
        if (ds_b) *ds_b = b;
    }
}

// ------------------------------------------------------------------------------------------ the byte table's sums
// d_byte[r, :] += the sum of the slab's d b rows whose id is r, as 64-bit FIXED POINT: a term is v * 2^k rounded to an integer, k
// from the slab's largest finite |v| (placed at 2^40, so that 2^20 terms per element and slab cannot overflow), and integer sums do
// not depend on the order of their adds -- in LDS (a workgroup owns a chunk of positions and a slice of columns that fits), in the
// flush of the LDS sums into the table `q` in global memory, or, where no slice of the table fits the LDS, in `q` directly.  The
// closing kernel converts, adds the slab's sums to d_byte (the slabs follow one another in stream order) and clears `q`.  A
// non-finite term takes a float atomic on d_byte itself: any order of infinities and NaNs gives the same result.
struct OnceByteArgs {
    const int64_t *ids;          // the slab's first position
    const float *dub;            // [n][bpt * Db]
    const uint32_t *gmax;        // the slab's word
    unsigned long long *q;       // [byte_rows][Db]
    float *d_byte;
    int64_t n;
    int byte_rows, bpt, Db, cw, chunk, use_lds;   // cw: columns per slice; chunk: positions per workgroup
};

__device__ __forceinline__ int once_fx_shift(uint32_t bits) {
    if (!bits) return 0;
    int e;
    frexpf(__uint_as_float(bits), &e);   // |v| < 2^e
    return 40 - e;
}

constexpr int kOnceByteThreads = 1024;   // 16 waves: with two workgroups per CU (64 KiB of LDS each) the loads of 32 waves cover one another's latency
__global__ __launch_bounds__(kOnceByteThreads) void once_byte_sums_kernel(const OnceByteArgs A) {
    extern __shared__ unsigned long long once_q[];   // [byte_rows][cw] with use_lds
    constexpr int U = 4;                             // items in flight per thread
    const int tid = threadIdx.x, Db = A.Db;
    const int c0 = blockIdx.y * A.cw, cw = min(A.cw, Db - c0), g4 = cw / 4;
    const int64_t p0 = (int64_t)blockIdx.x * A.chunk, p1 = min(A.n, p0 + A.chunk);
    const int k = once_fx_shift(*A.gmax);
    const int nq = A.byte_rows * A.cw;
    if (A.use_lds) {
        for (int i = tid; i < nq; i += kOnceByteThreads) once_q[i] = 0ull;
        __syncthreads();
    }
    const int items = (int)(p1 - p0) * A.bpt * g4;   // chunk * bpt * cw / 4 <= 512 * 64 * 512: fits
    const int64_t slot0 = p0 * A.bpt;                // (position, byte slot), flattened: the d b row of slot s lies at dub + s * Db
    for (int it0 = tid; it0 < items; it0 += U * kOnceByteThreads) {
        int id[U], c[U];
        float4v v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int it = min(it0 + u * kOnceByteThreads, items - 1);   // the tail re-reads the last item; its adds are skipped
            const int s = it / g4;
            c[u] = 4 * (it - s * g4);
            const int64_t r = A.ids[slot0 + s];
            id[u] = (uint64_t)r < (uint64_t)A.byte_rows ? (int)r : 0;    // flagged by pass A
            v[u] = *(const float4v *)(A.dub + (slot0 + s) * Db + c0 + c[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (it0 + u * kOnceByteThreads >= items) break;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = v[u][e];
                if (x == 0.f) continue;
                if (!(fabsf(x) < INFINITY)) { atomicAdd(A.d_byte + (int64_t)id[u] * Db + c0 + c[u] + e, x); continue; }
                // |x| 2^k < 2^40: the shift is exact in fp32, and so is the conversion
                const unsigned long long t = (unsigned long long)__float2ll_rn(ldexpf(x, k));
                if (A.use_lds) atomicAdd(once_q + id[u] * A.cw + c[u] + e, t);
                else atomicAdd(A.q + (int64_t)id[u] * Db + c0 + c[u] + e, t);
            }
        }
    }
    if (!A.use_lds) return;   // uniform over the workgroup
    __syncthreads();
    for (int i = tid; i < nq; i += kOnceByteThreads) {
        const int r = i / A.cw, cc = i - r * A.cw;
        const unsigned long long t = once_q[i];
        if (cc < cw && t) atomicAdd(A.q + (int64_t)r * Db + c0 + cc, t);
    }
}

__global__ __launch_bounds__(kThreads) void once_byte_close_kernel(unsigned long long *__restrict__ q, const uint32_t *__restrict__ gmax,
                                                                   float *__restrict__ d_byte, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long v = (long long)q[i];
    if (!v) return;
    d_byte[i] += (float)ldexp((double)v, -once_fx_shift(*gmax));
    q[i] = 0ull;
}

// ------------------------------------------------------------------------------------------ pass B
struct OnceSliceArgs {
    TokenSumsView V;            // the token order, the canonical positions and the pieces (mot_values.hip)
    int64_t N;
    int rows, Dt, nck, g_ld;    // nck: blocks of 64 16-byte chunks per token row; g_ld: elements between the rows of grad_out
    const void *g, *tok_table, *byte_table;
    void *d;
    const float4v *scal;
    const int64_t *ids;
    const float *byte_rnorm;
    const float *s_t, *s_b;
    int bpt, Db, byte_rows, norm_tok, norm_out;
};

__device__ __forceinline__ int once_row(int id, int rows) { return (uint32_t)id < (uint32_t)rows ? id : 0; }
__device__ __forceinline__ int once_pos(int p, int64_t N) { return (int)min((int64_t)max(p, 0), N - 1); }

// BYTES: the forward has a byte part in the token columns and an output norm, so x[cols] needs the byte-row piece (SUM with norm_out).
template <typename T, bool BYTES>
__global__ __launch_bounds__(kThreads) void once_slices_kernel(const OnceSliceArgs A) {
    typedef typename Elem<T>::vec vec_t;
    typedef typename Elem<T>::raw raw_t;
    constexpr int VEC = Elem<T>::kVec, U = 8;   // rows in flight per lane, whatever the groups' lengths
    const int lane = threadIdx.x & 63;
    const int64_t slice = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int64_t b = slice * kOnceSlice;
    if (b >= A.N) return;   // no barrier below
    const int ck = blockIdx.y;
    const int D = A.Dt, col = VEC * (ck * 64 + lane);
    const bool act = col < D;
    const int col0 = act ? col : 0;   // lanes past the row end re-read its first chunk: never stored
    const T *g = (const T *)A.g + col0;
    const T *tab = (const T *)A.tok_table + col0;
    T *dt = (T *)A.d + col;
    const bool need_a = A.norm_tok || A.norm_out;
    const float s_t = A.s_t ? *A.s_t : 1.f, s_b = A.s_b ? *A.s_b : 1.f;
    const int bk = BYTES ? col0 / A.Db : 0, bw = BYTES ? col0 - bk * A.Db : 0;   // the lane's byte slot and the chunk's place in its row
    const T *btab = (const T *)A.byte_table + bw;
    const int n = (int)min((int64_t)kOnceSlice, A.N - b);
    int myid = -1, myp = 0;
    float4v mysc = {1.f, 0.f, 1.f, 0.f};
    if (lane < n) {
        myid = once_row(A.V.id_sorted[b + lane], A.rows);
        myp = once_pos(A.V.canon[b + lane], A.N);
        if (need_a) mysc = A.scal[myp];
    }
    const int before = b > 0 ? once_row(A.V.id_sorted[b - 1], A.rows) : -1;
    const int after = b + n < A.N ? once_row(A.V.id_sorted[b + n], A.rows) : -1;
    // bit t: slot t is the last one of its group's run in this slice (lanes past the slice hold -1, so slot n - 1 always is)
    const int next_id = __shfl_down(myid, 1);   // by every lane: a lane left out of the shuffle hands nothing to its neighbour
    const unsigned long long ends = __ballot(lane < n && (lane == 63 || next_id != myid));
    vec_t acc = {};
    int m = 0;   // the first slot of the current run
    for (int t0 = 0; t0 < n; t0 += U) {
        raw_t gr[U], ar[U], br[U];
        float rk[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int tt = min(t0 + u, n - 1);
            const int64_t p = __shfl(myp, tt);
            gr[u] = Elem<T>::load_raw(g + p * A.g_ld);
            if (need_a) {   // the group's token-row piece: one address for the whole group, so all but its first request hit L1 / L2
                const int id = __shfl(myid, tt);
                ar[u] = Elem<T>::load_raw(tab + (int64_t)id * D);
            }
            if (BYTES) {
                int64_t bid = A.ids[p * A.bpt + bk];
                if ((uint64_t)bid >= (uint64_t)A.byte_rows) bid = 0;   // flagged by pass A
                rk[u] = A.byte_rnorm ? A.byte_rnorm[bid] : 1.f;
                br[u] = Elem<T>::load_raw(btab + bid * A.Db);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u;
            if (t >= n) break;
            vec_t da = Elem<T>::widen(gr[u]);
            if (need_a) {
                const float r_o = __shfl(mysc.x, t), c_o = __shfl(mysc.y, t), r_t = __shfl(mysc.z, t), c_t = __shfl(mysc.w, t);
                const vec_t ah = Elem<T>::widen(ar[u]) * r_t;   // a^ (r_t = 1 without norm_tok)
                if (A.norm_out) {
                    vec_t y = ah * s_t;
                    if (BYTES) y += Elem<T>::widen(br[u]) * (rk[u] * s_b);
                    da = (da - y * (r_o * c_o)) * r_o;   // dy
                }
                da = (da * s_t - ah * c_t) * r_t;   // (c_t = 0, r_t = 1 without norm_tok)
            } else {
                da *= s_t;
            }
            acc += da;
            if (!((ends >> t) & 1ull)) continue;
            const int id = __shfl(myid, t);
            const bool opens = m > 0 || id != before;        // the group's first position is in this slice
            const bool closes = t + 1 < n || id != after;    // and its last one
            if (act) {
                if (opens && closes) {
                    Elem<T>::storev_nt(dt + (int64_t)id * D, acc);
                } else {
                    float *p = A.V.part + ((int64_t)slice * 2 + (opens ? 1 : 0)) * (int64_t)D + col;
                    *(vec_t *)p = acc;
                }
            }
            acc = vec_t{};
            m = t + 1;
        }
    }
}

// ------------------------------------------------------------------------------------------ validation (no HIP call)
static bool once_has_bytes(const MotEmbedMixDesc &d) { return d.mode != MOT_MIX_NOOP; }

// everything that does not need the pointers: also what the size query runs
static int once_check_shape(const MotEmbedMixDesc *d) {
    if (!d) return set_error(MOT_EINVAL, "embed_mix_bwd_once: null descriptor");
    if (d->struct_size != sizeof(MotEmbedMixDesc))
        return set_error(MOT_EINVAL, "embed_mix_bwd_once: struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(MotEmbedMixDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EINVAL, "embed_mix_bwd_once: bad dtype %d", d->dtype);
    if (d->reserved0) return set_error(MOT_EINVAL, "embed_mix_bwd_once: reserved0 %u", d->reserved0);
    if (d->mode == MOT_MIX_CONCAT_LINEAR)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: MOT_MIX_CONCAT_LINEAR is not built here (follow-up: form d u = dy W in token order; "
                                           "mot_embed_mix_bwd has this mode)");
    if (d->mode == MOT_MIX_MEAN)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: MOT_MIX_MEAN is not built here (follow-up: its small table takes the dense product of "
                                           "mot_embed_mix_bwd, which has this mode)");
    if (d->mode != MOT_MIX_NOOP && d->mode != MOT_MIX_SUM && d->mode != MOT_MIX_CONCAT) return set_error(MOT_EINVAL, "embed_mix_bwd_once: bad mode %d", d->mode);
    if (d->id_source == MOT_IDS_FROM_TTB)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: MOT_IDS_FROM_TTB is not built here (follow-up: the index phase in the backward); pass the "
                                           "byte ids the forward returned (MOT_IDS_GIVEN)");
    if (once_has_bytes(*d) && d->ids_b)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: a second id tensor (ids_b) is not built here (follow-up: the sum of two byte rows in both "
                                           "passes; mot_embed_mix_bwd has it)");
    if (once_has_bytes(*d) && d->id_source != MOT_IDS_GIVEN) return set_error(MOT_EINVAL, "embed_mix_bwd_once: bad id_source %d", d->id_source);
    if (d->n_rows < 0 || d->tokens_per_row < 0) return set_error(MOT_ESHAPE, "embed_mix_bwd_once: negative shape");
    if (d->tok_rows <= 0 || d->tok_dim <= 0 || d->model_dim <= 0) return set_error(MOT_ESHAPE, "embed_mix_bwd_once: empty token table");
    const int vec = d->dtype == MOT_BF16 ? 8 : 4;
    if (once_has_bytes(*d)) {
        if (d->bpt < 1 || d->bpt > MOT_MAX_BPT)
            return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: bytes_per_token %d outside [1, %d]", d->bpt, MOT_MAX_BPT);
        if (d->byte_rows <= 0 || d->byte_dim <= 0) return set_error(MOT_ESHAPE, "embed_mix_bwd_once: empty byte table");
        if (d->byte_rows > 0x7fffffffLL / d->byte_dim) return set_error(MOT_ESHAPE, "embed_mix_bwd_once: a byte table of %lld rows", (long long)d->byte_rows);
        if (d->byte_dim % vec)
            return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: byte_dim %d must be a multiple of %d elements (16 bytes)", d->byte_dim, vec);
    }
    if (d->tok_dim % vec) return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: tok_dim %d must be a multiple of %d elements (16 bytes)", d->tok_dim, vec);
    const int64_t nbk = once_has_bytes(*d) ? (int64_t)d->bpt * d->byte_dim : 0;
    if (d->mode == MOT_MIX_SUM && (nbk != d->tok_dim || d->model_dim != d->tok_dim))
        return set_error(MOT_ESHAPE, "embed_mix_bwd_once sum: need bpt*byte_dim == tok_dim == model_dim (got %d*%d, %d, %d)", d->bpt, d->byte_dim, d->tok_dim,
                         d->model_dim);
    if (d->mode == MOT_MIX_NOOP && d->model_dim != d->tok_dim)
        return set_error(MOT_ESHAPE, "embed_mix_bwd_once noop: model_dim %d != tok_dim %d", d->model_dim, d->tok_dim);
    if (d->mode == MOT_MIX_CONCAT) {
        if (d->weight || d->bias) return set_error(MOT_EINVAL, "embed_mix_bwd_once concat: the pure concatenation takes no weight / bias");
        if ((int64_t)d->model_dim != d->tok_dim + nbk)
            return set_error(MOT_ESHAPE, "embed_mix_bwd_once concat: need model_dim == tok_dim + bpt*byte_dim (got %d, %d + %d*%d)", d->model_dim, d->tok_dim,
                             d->bpt, d->byte_dim);
    }
    if (d->model_dim > kOnceMaxDim) return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: model_dim %d > %d is not built", d->model_dim, kOnceMaxDim);
    if (d->tok_rows >= kOnceOrderLimit)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: token tables of %lld rows (>= 2^21 - 1, the token order's limit) are not built",
                         (long long)d->tok_rows);
    if (d->n_rows * d->tokens_per_row > 0x7fffffffLL || d->tokens_per_row * (int64_t)(d->bpt > 0 ? d->bpt : 1) > 0x7fffffffLL)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd_once: T*bpt or B*T exceeds 2^31");
    return MOT_OK;
}

// workspace: [byte rows' rms factors][{r_o, c_o, r_t, c_t}: 16 bytes per position][scalar partials: 2 per 16 positions]
//            [token sums: order, canon, slice pieces][d b: one slab x bpt * byte_dim fp32][the byte table's fixed-point sums: 8 bytes per
//            element][a word per slab]
struct OnceLayout { size_t rnorm, scal, part, sums, dub, q, gmax, total; int64_t slab, nblk, nslab; };
static OnceLayout once_layout(const MotEmbedMixDesc &d) {
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row);
    const bool bytes = once_has_bytes(d);
    OnceLayout L{};
    L.slab = (int64_t)(N < (size_t)kOnceSlab ? N : (size_t)kOnceSlab);
    L.nblk = (int64_t)((N + kOnceBlockTok - 1) / kOnceBlockTok);
    Arena ar;
    L.rnorm = ar.take(bytes ? (size_t)d.byte_rows * sizeof(float) : 0);
    L.scal = ar.take(N * sizeof(float4v));
    L.part = ar.take((size_t)L.nblk * 2 * sizeof(float));
    L.sums = ar.take(token_sums_ws_bytes((int64_t)N, d.tok_rows, d.tok_dim, d.dtype));
    L.dub = ar.take(bytes ? (size_t)L.slab * d.bpt * d.byte_dim * sizeof(float) : 0);
    L.nslab = L.slab ? (int64_t)((N + L.slab - 1) / L.slab) : 0;
    L.q = ar.take(bytes ? (size_t)d.byte_rows * d.byte_dim * sizeof(unsigned long long) : 0);
    L.gmax = ar.take(bytes ? (size_t)L.nslab * sizeof(uint32_t) : 0);
    L.total = ar.o;
    return L;
}

size_t embed_mix_bwd_once_workspace_bytes(const MotEmbedMixDesc *d) {
    if (once_check_shape(d)) return 0;
    if (d->n_rows == 0 || d->tokens_per_row == 0) return 0;
    return once_layout(*d).total;
}

int embed_mix_bwd_once_check(const MotEmbedMixDesc *d, const MotEmbedMixGradsOnce *g) {
    if (!g || g->struct_size != sizeof(MotEmbedMixGradsOnce))
        return set_error(MOT_EINVAL, "embed_mix_bwd_once: grads struct missing or struct_size mismatch");
    if (int rc = once_check_shape(d)) return rc;
    if (g->reserved) return set_error(MOT_EINVAL, "embed_mix_bwd_once: reserved %u", g->reserved);
    if (!d->tokens || !d->tok_table) return set_error(MOT_EINVAL, "embed_mix_bwd_once: tokens / tok_table must be non-null");
    if (once_has_bytes(*d) && (!d->byte_table || !d->ids_a)) return set_error(MOT_EINVAL, "embed_mix_bwd_once: byte_table / ids_a must be non-null");
    if (!g->grad_out) return set_error(MOT_EINVAL, "embed_mix_bwd_once: grad_out missing");
    if (!once_has_bytes(*d) && g->d_byte_table) return set_error(MOT_EINVAL, "embed_mix_bwd_once: d_byte_table given, but MOT_MIX_NOOP has no byte table");
    const uintptr_t align = (uintptr_t)d->tok_table | (uintptr_t)d->byte_table | (uintptr_t)g->grad_out | (uintptr_t)g->d_tok_table | (uintptr_t)g->d_byte_table;
    if (align & 15) return set_error(MOT_EINVAL, "embed_mix_bwd_once: tables and gradients must be 16-byte aligned");
    if (d->n_rows == 0 || d->tokens_per_row == 0) return MOT_OK;
    return check_workspace("embed_mix_bwd_once", false, d->workspace, d->workspace ? d->workspace_bytes : (size_t)0, once_layout(*d).total);
}

// ------------------------------------------------------------------------------------------ launches
template <typename T>
static void launch_once_rows(const OnceRowsArgs &A, unsigned nb, int nch, hipStream_t stream) {
    constexpr int kMid = sizeof(T) == 2 ? 2 : 4, kTop = 2 * kMid;   // bf16: 1, 2, 4 chunks per lane; fp32: 1, 4, 8
    if (nch <= 1) hipLaunchKernelGGL((once_rows_kernel<T, 1>), dim3(nb), dim3(kThreads), 0, stream, A);
    else if (nch <= kMid) hipLaunchKernelGGL((once_rows_kernel<T, kMid>), dim3(nb), dim3(kThreads), 0, stream, A);
    else hipLaunchKernelGGL((once_rows_kernel<T, kTop>), dim3(nb), dim3(kThreads), 0, stream, A);
}

int launch_embed_mix_bwd_once(const MotEmbedMixDesc &d, const MotEmbedMixGradsOnce &gr, hipStream_t stream) {
    const int64_t N = d.n_rows * d.tokens_per_row;
    const bool bf = d.dtype == MOT_BF16, bytes = once_has_bytes(d);
    const int vec = bf ? 8 : 4;
    const size_t esz = bf ? 2 : 4;
    const int D = d.model_dim, Dt = d.tok_dim, Db = bytes ? d.byte_dim : 0, bpt = bytes ? d.bpt : 0;
    const float eps = d.eps > 0.f ? d.eps : (bf ? kBf16Eps : FLT_EPSILON);   // as mot_embed_mix_fwd / mot_embed_mix_bwd
    const bool want_scalars = gr.d_scale_tok || gr.d_scale_byte;
    const bool want_byte = bytes && gr.d_byte_table;
    if (!gr.d_tok_table && !want_byte && !want_scalars) return MOT_OK;
    const OnceLayout L = once_layout(d);
    char *ws = (char *)d.workspace;
    float *rnorm = (float *)(ws + L.rnorm), *part = (float *)(ws + L.part), *dub = (float *)(ws + L.dub);
    float4v *scal = (float4v *)(ws + L.scal);
    const bool norm_byte = bytes && d.norm_byte;
    int rc;
    if (norm_byte && (rc = launch_rows_rnorm(d.byte_table, d.byte_rows, Db, eps, rnorm, d.dtype, stream))) return rc;
    unsigned long long *q = (unsigned long long *)(ws + L.q);
    uint32_t *gmax = (uint32_t *)(ws + L.gmax);
    // the byte table's slices: the widest multiple of four columns whose 64-bit sums of every row fit 64 KiB of LDS (two workgroups per CU)
    int cw = bytes ? (int)((64 * 1024 / sizeof(unsigned long long) / (size_t)d.byte_rows) & ~(size_t)3) : 0;
    const int use_lds = cw >= 4;
    if (!use_lds || cw > Db) cw = Db;
    if (want_byte) {   // kernels, not memset nodes; q and the slabs' words are one piece of the workspace
        if ((rc = launch_zero_words(gr.d_byte_table, d.byte_rows * Db, stream))) return rc;
        if ((rc = launch_zero_words(q, (int64_t)((L.gmax - L.q) / 4 + L.nslab), stream))) return rc;
    }
    // pass A: needed for the norms' per-position scalars, the byte part and the scale gradients
    if (d.norm_tok || d.norm_out || want_byte || want_scalars) {
        for (int64_t r0 = 0; r0 < N; r0 += L.slab) {   // (the slab is a whole number of workgroups' positions)
            const int64_t n = N - r0 < L.slab ? N - r0 : L.slab;
            OnceRowsArgs A{};
            A.tokens = d.tokens + r0; A.ids = bytes ? d.ids_a + r0 * bpt : nullptr;
            A.tok_table = d.tok_table; A.byte_table = d.byte_table; A.byte_rnorm = norm_byte ? rnorm : nullptr;
            A.g = (const char *)gr.grad_out + (size_t)r0 * D * esz;
            A.s_t = d.scale_tok; A.s_b = d.scale_byte;
            A.scal = scal + r0;
            A.dub = want_byte ? dub : nullptr;
            A.part = want_scalars ? part + 2 * (r0 / kOnceBlockTok) : nullptr;
            A.gmax = gmax + r0 / L.slab;
            A.n = n; A.tok_rows = (int)d.tok_rows; A.byte_rows = (int)d.byte_rows; A.bpt = bpt; A.Db = Db; A.Dt = Dt; A.D = D;
            A.mode = d.mode; A.norm_tok = d.norm_tok; A.norm_out = d.norm_out; A.eps = eps; A.status = d.status;
            const unsigned nb = (unsigned)((n + kOnceBlockTok - 1) / kOnceBlockTok);
            const int nch = (D / vec + 63) / 64;
            if (bf) launch_once_rows<__bf16>(A, nb, nch, stream);
            else launch_once_rows<float>(A, nb, nch, stream);
            if ((rc = check_launch("once_rows_kernel"))) return rc;
            if (!want_byte) continue;
            // d_byte += the slab's d b rows
            OnceByteArgs Y{};
            Y.ids = A.ids; Y.dub = dub; Y.gmax = A.gmax; Y.q = q; Y.d_byte = gr.d_byte_table;
            Y.n = n; Y.byte_rows = (int)d.byte_rows; Y.bpt = bpt; Y.Db = Db; Y.cw = cw; Y.chunk = kOnceByteChunk; Y.use_lds = use_lds;
            const dim3 yg((unsigned)((n + kOnceByteChunk - 1) / kOnceByteChunk), (unsigned)((Db + cw - 1) / cw));
            const size_t lds = use_lds ? (size_t)d.byte_rows * cw * sizeof(unsigned long long) : 0;
            static std::atomic<uint64_t> lds_ok{0};   // per-device bits
            if (lds > 48 * 1024)
                if ((rc = ensure_max_dyn_lds((const void *)once_byte_sums_kernel, lds_ok, "once_byte_sums_kernel"))) return rc;
            hipLaunchKernelGGL(once_byte_sums_kernel, yg, dim3(kOnceByteThreads), lds, stream, Y);
            const int64_t nel = d.byte_rows * Db;
            hipLaunchKernelGGL(once_byte_close_kernel, dim3((unsigned)((nel + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, q, A.gmax, gr.d_byte_table, nel);
            if ((rc = check_launch("once_byte_sums_kernel / once_byte_close_kernel"))) return rc;
        }
        if (want_scalars) {
            hipLaunchKernelGGL(once_scalars_kernel, dim3(1), dim3(kOnceSumThreads), 0, stream, part, L.nblk, gr.d_scale_tok, gr.d_scale_byte);
            if ((rc = check_launch("once_scalars_kernel"))) return rc;
        }
    }
    if (!gr.d_tok_table) return MOT_OK;
    // pass B: the order and the canonical positions, the formed rows summed slice by slice, the closing rows kernel
    OnceSliceArgs S{};
    if ((rc = launch_token_canon(d.tokens, N, d.tok_rows, Dt, d.dtype, gr.token_order, ws + L.sums, d.status, stream, &S.V))) return rc;
    S.N = N; S.rows = (int)d.tok_rows; S.Dt = Dt; S.nck = (Dt / vec + 63) / 64; S.g_ld = D;
    S.g = gr.grad_out; S.tok_table = d.tok_table; S.byte_table = d.byte_table; S.d = gr.d_tok_table;
    S.scal = scal; S.ids = d.ids_a; S.byte_rnorm = norm_byte ? rnorm : nullptr;
    S.s_t = d.scale_tok; S.s_b = d.scale_byte;
    S.bpt = bpt; S.Db = Db > 0 ? Db : 1; S.byte_rows = (int)d.byte_rows; S.norm_tok = d.norm_tok; S.norm_out = d.norm_out;
    const bool with_bytes = d.mode == MOT_MIX_SUM && d.norm_out;
    const int64_t slices = (N + kOnceSlice - 1) / kOnceSlice;
    const dim3 sg((unsigned)((slices + kWaves - 1) / kWaves), (unsigned)S.nck);
    if (bf) {
        if (with_bytes) hipLaunchKernelGGL((once_slices_kernel<__bf16, true>), sg, dim3(kThreads), 0, stream, S);
        else hipLaunchKernelGGL((once_slices_kernel<__bf16, false>), sg, dim3(kThreads), 0, stream, S);
    } else {
        if (with_bytes) hipLaunchKernelGGL((once_slices_kernel<float, true>), sg, dim3(kThreads), 0, stream, S);
        else hipLaunchKernelGGL((once_slices_kernel<float, false>), sg, dim3(kThreads), 0, stream, S);
    }
    if ((rc = check_launch("once_slices_kernel"))) return rc;
    return launch_token_rows_close(S.V, N, d.tok_rows, Dt, d.dtype, gr.d_tok_table, stream);
}

}  // namespace mot
