// mot_splitx0.hip -- the three input streams of modded-nanogpt/runs/71081_mot-in_toks-valemb.py:302-304, 315 in one call:
//     x0t = norm(embed_tokens(tok))                      (T, D)   norm over D = token_dim
//     x0b = cat_k norm(embed_bytes(ids[:, k]))           (T, D)   norm over byte_dim, per byte row, BEFORE the cat; D = bpt * byte_dim
//     x   = x0t * scalars[-1] + x0b * scalars[-2]        (T, D)   no outer norm
// forward and backward, fp32 and bf16 (include/mot.h, MotSplitX0Desc).  Every block of the run reads all three (:209-210, :319).
//
// Forward (split_x0_fwd_kernel, ONE launch for all requested outputs, behind the per-call table of the byte rows' rms factors:
// launch_rows_rnorm, byte_rows floats -- a byte row's factor depends on its id only, and a row's byte_dim / VEC chunks are not a
// power-of-two group of lanes at 48 or 24 columns, so the table replaces a segmented reduction per (token, slot)): a wave owns a
// unit of 16 or 32 consecutive tokens of one row and runs the index phase of the fused front-end (mot_wave.hpp: WaveIndexer /
// wave_ids_given, unchanged), which leaves the unit's ids in wave-private LDS.  Lane l owns the 16-byte chunks l, l + 64, ... of a
// row.  The token row comes in as coalesced wave loads from a wave-uniform row number, its sum of squares
// is the six-step DPP wave reduction; the byte chunk and its factor come from L2.  A lane then holds, per chunk, the x0t piece, the
// x0b piece and s_t x0t + s_b x0b, and stores each requested output with non-temporal 16-byte stores.  Arithmetic is fp32; bf16 is
// rounded where the reference's eager bf16 run rounds: x0t = bf16(r_t a), x0b = bf16(r_k u_k), x = bf16(bf16(s_t x0t) + bf16(s_b x0b))
// from the ROUNDED x0t and x0b.  Algorithmic bytes per token: 4 + 2 bpt (ids from the token->byte table) or 4 + 8 bpt (ids given)
// + e D read, n_out e D written.
//
// Resources of every instantiation, from the compiler's own remarks (-Rpass-analysis=kernel-resource-usage, gfx950; forward
// <T, NCH, U>: VGPRs / SGPRs / scratch bytes per lane / waves per SIMD):
//     <bf16, 1, 4>   72 / 106 / 0 / 7      <bf16, 2, 2>   89 / 106 / 0 / 5      <bf16, 4, 1>  101 / 106 / 0 / 4
//     <fp32, 1, 4>   62 / 106 / 0 / 7      <fp32, 4, 1>   85 / 106 / 0 / 5      <fp32, 8, 1>  140 / 106 / 0 / 3
//   split_x0_rows_kernel <T, NCH>:
//     <bf16, 1>      74 /  93 / 0 / 6      <bf16, 2>      90 / 106 / 0 / 5      <bf16, 4>     147 / 106 / 0 / 3
//     <fp32, 1>      54 /  87 / 0 / 8      <fp32, 4>      86 / 106 / 0 / 5      <fp32, 8>     153 / 106 / 0 / 3
//   split_x0_scalars_kernel 34 / 18 / 0 / 8.
// No instantiation uses scratch.  The token rows are requested BEHIND the index phase: requested in front of it, as the fused
// front-end does, they held enough scalar registers across the six inlined indexers that the compiler set a 36-byte private
// segment aside in three of the six instantiations.
//
// Backward, one call, everything recomputed from the tables (nothing of the forward is saved but the ids).  With
// h_t = g_x0t + s_t g_x and h_b = g_x0b + s_b g_x (absent gradients are zero):
//   split_x0_rows_kernel     a wave per token, four tokens one after the other: d a_n = r_t (h_t - x0t (h_t . x0t) / D) and
//                            d u_{n,k} = r_k (h_b[k] - y_k (h_b[k] . y_k) / byte_dim) as fp32 rows into the workspace (the per-slot
//                            dots through wave-private LDS: a partial per chunk, one lane per slot adds its slot's in chunk order), and
//                            the workgroup's partial of d s_t = sum g_x . x0t and d s_b = sum g_x . x0b over its 16 positions
//                            (lanes over the wave's tokens, the DPP reduction, then the four waves in wave order);
//   token table              the fp32 rows of the WHOLE batch go through the order, canon, slices and rows kernels of the token
//                            value embeddings (launch_token_sums_f32, mot_values.hip): written once in the table's dtype, fp32 sums
//                            in ascending position order, +0 rows for absent ids, no atomics, the same bits on every run;
//   byte table               slab by slab (16 384 positions) through the LDS fixed-point sums of the byte value embeddings
//                            (launch_byte_cat_bwd as an un-normed fp32 byte_cat, mot_bytecat.hip, unchanged): fp32, +=;
//   split_x0_scalars_kernel  ONE workgroup adds the partials in order: thread t its contiguous share, thread 0 the 256 shares.
//                            The grid of the row kernel depends on the shape only, so d s_t and d s_b are the same bits on every run.
#include <type_traits>

#include "mot_wave.hpp"

namespace mot {

constexpr int kSxMaxDim = 2048;
constexpr int64_t kSxSlab = 16384;          // positions per slab of the byte part's fp32 rows: 64 MiB at D 1024
constexpr int kSxTok = 4;                   // positions per wave of the row kernel
constexpr int kSxBlockTok = kSxTok * kWaves;   // positions per workgroup: one pair of scalar partials each
constexpr int kSxOrderLimit = (1 << 21) - 1;   // the token order's limit on the table height (mot_group.hip)

struct SplitArgs {
    MixArgs M;   // ids, tables, eps, the two scalars and the byte rows' factors (what WaveIndexer / wave_ids_given read is in here)
    void *x0t, *x0b, *x;
    int Dm;
};

// a value as the output dtype holds it, widened again
template <typename T, typename V> __device__ __forceinline__ V sx_round(V v) {
    if constexpr (std::is_same<T, __bf16>::value) return __builtin_convertvector(__builtin_convertvector(v, bf16x8v), float8v);
    else return v;
}

// ------------------------------------------------------------------------------------------ forward
// The token rows of a batch of U tokens in flight: lane unit_lane0 + j of `tokv` holds token j of the unit.
template <typename T, int NCH, int U>
struct SxTokenRows {
    typedef typename Elem<T>::raw raw_t;
    static constexpr int VEC = Elem<T>::kVec;
    const MixArgs &A;
    const T *tok_lane;   // the table at the lane's first chunk: a per-lane pointer, so the row bases stay out of the scalar registers
    int Dm, nchunk, lane, ntok;
    int tokv = 0, unit_lane0 = 0;
    raw_t ar[U][NCH];
    __device__ __forceinline__ void request(int tb) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = min(tb + u, ntok - 1);   // the tail re-reads the last token; its store is skipped
            int tok = __builtin_amdgcn_readlane(tokv, unit_lane0 + t);   // wave-uniform: the row's address is scalar
            if ((uint64_t)(uint32_t)tok >= (uint64_t)A.tok_rows) {
                if (A.status && lane == 0) atomicOr(A.status, kStatusTokenOor);
                tok = 0;
            }
            const T *trow = tok_lane + (int64_t)tok * Dm;
#pragma unroll
            for (int i = 0; i < NCH; ++i) ar[u][i] = Elem<T>::load_raw(trow + VEC * (lane + 64 * i < nchunk ? 64 * i : -lane));   // lanes past the row end re-read its first chunk
        }
    }
};

// NCH: 16-byte chunks per lane (covers Dm <= 64 * NCH * VEC).  U: tokens in flight per wave (a token row and a byte row each).
template <typename T, int NCH, int U>
__global__ __launch_bounds__(kThreads) void split_x0_fwd_kernel(const SplitArgs S) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_wave[];
    typedef typename Elem<T>::vec vec_t;
    typedef typename Elem<T>::raw raw_t;
    constexpr int VEC = Elem<T>::kVec;
    const MixArgs &A = S.M;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit_id = (int64_t)blockIdx.x * kWaves + wave;
    if (unit_id >= A.n_units) return;   // no barrier anywhere below: a wave may leave on its own
    const int64_t row = unit_id / A.units_per_row;
    const int64_t u0 = (unit_id - row * A.units_per_row) * A.unit;
    const int ntok = (int)min((int64_t)A.unit, A.T - u0);
    const int stream_eb = (A.id_source == MOT_IDS_FROM_TTB && A.pull_dir != kPullNone) ? A.ttb_elem : 0;
    const WaveLds W = wave_lds_carve(lds_wave + (size_t)wave * A.wave_lds, A.unit, A.bpt, false, stream_eb);

    const int Dm = S.Dm, Db = A.Db, nchunk = Dm / VEC, sv = A.bpt | 1;
    const T *byte_table = (const T *)A.byte_table;
    SxTokenRows<T, NCH, U> R{A, (const T *)A.tok_table + VEC * lane, Dm, nchunk, lane, ntok};

    // ---- the unit's byte ids into wave-private LDS
    auto from_ttb = [&](auto indexer) {
        R.tokv = indexer.tokens();
        R.unit_lane0 = indexer.unit_lane0;
        indexer.load_rows();
        indexer.finish();
    };
    if (A.id_source == MOT_IDS_FROM_TTB) {
        if (A.ttb_elem == 2) {
            if (A.pull_dir == kPullLeft) from_ttb(WaveIndexer<kPullLeft, int16_t>(A, W, row, u0, ntok, false));
            else if (A.pull_dir == kPullRight) from_ttb(WaveIndexer<kPullRight, int16_t>(A, W, row, u0, ntok, false));
            else from_ttb(WaveIndexer<kPullNone, int16_t>(A, W, row, u0, ntok, false));
        } else {
            if (A.pull_dir == kPullLeft) from_ttb(WaveIndexer<kPullLeft, int32_t>(A, W, row, u0, ntok, false));
            else if (A.pull_dir == kPullRight) from_ttb(WaveIndexer<kPullRight, int32_t>(A, W, row, u0, ntok, false));
            else from_ttb(WaveIndexer<kPullNone, int32_t>(A, W, row, u0, ntok, false));
        }
    } else {
        R.tokv = lane < ntok ? A.tokens[row * A.T + u0 + lane] : 0;
        wave_ids_given(A, W, row, u0, ntok);
    }

    // ---- streaming: column VEC * c of a row belongs to byte slot VEC * c / Db (the cat of :304)
    bool act[NCH];
    int slot[NCH], within[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int c = lane + 64 * i;
        act[i] = c < nchunk;
        const int cc = act[i] ? c : 0;   // lanes past the row end re-read its first chunk: kept out of the sums, never stored
        slot[i] = (VEC * cc) / Db;
        within[i] = VEC * cc - slot[i] * Db;
    }
    const float s_t = *A.scale_tok, s_b = *A.scale_byte;
    const int64_t at0 = (row * A.T + u0) * (int64_t)Dm + VEC * lane;   // per-lane output pointers, likewise
    T *o_t = S.x0t ? (T *)S.x0t + at0 : nullptr;
    T *o_b = S.x0b ? (T *)S.x0b + at0 : nullptr;
    T *o_x = S.x ? (T *)S.x + at0 : nullptr;
    for (int tb = 0; tb < ntok; tb += U) {
        raw_t br[U][NCH];
        float rk[U][NCH];
        R.request(tb);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = min(tb + u, ntok - 1);
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int id = W.ids[t * sv + slot[i]];   // clamped to the byte table by the index phase
                br[u][i] = Elem<T>::load_raw(byte_table + (int64_t)id * Db + within[i]);
                rk[u][i] = A.byte_rnorm[id];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = tb + u;
            vec_t a[NCH];
            float ss = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                a[i] = Elem<T>::widen(R.ar[u][i]);
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < VEC; ++e) s += a[i][e] * a[i][e];
                ss += act[i] ? s : 0.f;
            }
            const float r = rms_scale(wave_sum(ss), Dm, A.eps);
            if (t < ntok) {
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    if (!act[i]) continue;
                    const int64_t at = (int64_t)t * Dm + VEC * 64 * i;
                    const vec_t xt = sx_round<T>(a[i] * r), xb = sx_round<T>(Elem<T>::widen(br[u][i]) * rk[u][i]);
                    if (o_t) Elem<T>::storev_nt(o_t + at, xt);
                    if (o_b) Elem<T>::storev_nt(o_b + at, xb);
                    if (o_x) Elem<T>::storev_nt(o_x + at, sx_round<T>(xt * s_t) + sx_round<T>(xb * s_b));
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ backward
struct SplitBwdArgs {
    const int32_t *tokens;      // the launch's first position
    const int64_t *ids;
    const void *tok_table, *byte_table;
    const float *byte_rnorm;
    const void *g_t, *g_b, *g_x;   // the launch's first row of each, or null
    const float *s_t, *s_b;
    float *da;                  // [n][D] fp32 or null
    float *dub;                 // [n][D] fp32 or null
    float *part;                // [blocks][2] of this launch, or null
    int64_t n;
    int tok_rows, byte_rows, bpt, Db, D;
    float eps;
    uint32_t *status;
};

// NCH: 16-byte chunks per lane (covers D <= 64 * NCH * VEC), as in the forward.
template <typename T, int NCH>
__global__ __launch_bounds__(kThreads) void split_x0_rows_kernel(const SplitBwdArgs A) {
    typedef typename Elem<T>::vec vec_t;
    constexpr int VEC = Elem<T>::kVec;
    __shared__ float parts[kWaves][kSxMaxDim / 4];   // a chunk's share of its slot's dot
    __shared__ float dots[kWaves][kMaxBpt];
    __shared__ float red[kWaves][2];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int D = A.D, Db = A.Db, bpt = A.bpt, nv = D / VEC, L = Db / VEC;
    const T *tok_table = (const T *)A.tok_table, *byte_table = (const T *)A.byte_table;
    const T *g_t = (const T *)A.g_t, *g_b = (const T *)A.g_b, *g_x = (const T *)A.g_x;
    const float s_t = *A.s_t, s_b = *A.s_b;
    const bool tok_part = A.da || A.part, byte_part = A.dub || A.part;
    const float inv_D = 1.0f / (float)D, inv_Db = 1.0f / (float)Db;
    float acc_t = 0.f, acc_b = 0.f;   // the lane's share of d s_t and d s_b over the wave's positions
    const int64_t n0 = ((int64_t)blockIdx.x * kWaves + wave) * kSxTok;
    for (int q = 0; q < kSxTok; ++q) {
        const int64_t n = n0 + q;
        if (n >= A.n) break;   // wave-uniform; the barrier is behind the loop
        if (tok_part) {
            int tok = A.tokens[n];
            if ((uint64_t)(uint32_t)tok >= (uint64_t)A.tok_rows) {
                if (A.status && lane == 0) atomicOr(A.status, kStatusTokenOor);
                tok = 0;
            }
            const T *arow = tok_table + (int64_t)tok * D;
            vec_t a[NCH], h[NCH];
            float ss = 0.f, ga = 0.f;   // ga: the lane's share of g_x . a (x0t = r a, and r is wave-uniform)
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int j = lane + 64 * i;
                a[i] = (vec_t)(0.f); h[i] = (vec_t)(0.f);
                if (j < nv) {
                    a[i] = Elem<T>::loadv(arow + VEC * j);
                    vec_t gx = (vec_t)(0.f);
                    if (g_x) gx = Elem<T>::loadv(g_x + n * D + VEC * j);
                    if (g_t) h[i] = Elem<T>::loadv(g_t + n * D + VEC * j);
                    h[i] += gx * s_t;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) { ss += a[i][e] * a[i][e]; ga += gx[e] * a[i][e]; }
                }
            }
            const float r = rms_scale(wave_sum(ss), D, A.eps);
            acc_t += r * ga;
            float m = 0.f;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                a[i] *= r;   // x0t
#pragma unroll
                for (int e = 0; e < VEC; ++e) m += h[i][e] * a[i][e];
            }
            m = wave_sum(m) * inv_D;
            if (A.da) {
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    const int j = lane + 64 * i;
                    if (j < nv) *(vec_t *)(A.da + n * D + VEC * j) = (h[i] - a[i] * m) * r;
                }
            }
        }
        if (byte_part) {
            vec_t y[NCH], h[NCH];
            float rk[NCH];
            int kk[NCH];
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int j = lane + 64 * i;
                y[i] = (vec_t)(0.f); h[i] = (vec_t)(0.f); rk[i] = 0.f; kk[i] = 0;
                if (j < nv) {
                    const int k = (VEC * j) / Db, w = VEC * j - k * Db;
                    int64_t id = A.ids[n * bpt + k];
                    if ((uint64_t)id >= (uint64_t)A.byte_rows) { if (A.status) atomicOr(A.status, kStatusByteOor); id = 0; }
                    kk[i] = k;
                    rk[i] = A.byte_rnorm[id];
                    y[i] = Elem<T>::loadv(byte_table + id * Db + w) * rk[i];
                    vec_t gx = (vec_t)(0.f);
                    if (g_x) gx = Elem<T>::loadv(g_x + n * D + VEC * j);
                    if (g_b) h[i] = Elem<T>::loadv(g_b + n * D + VEC * j);
                    h[i] += gx * s_b;
                    float p = 0.f;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) { p += h[i][e] * y[i][e]; acc_b += gx[e] * y[i][e]; }
                    parts[wave][j] = p;
                }
            }
            if (A.dub) {
                wave_lds_sync();
                if (lane < bpt) {   // one lane per slot: its L chunks in chunk order
                    float s = 0.f;
                    for (int c = 0; c < L; ++c) s += parts[wave][lane * L + c];
                    dots[wave][lane] = s * inv_Db;
                }
                wave_lds_sync();
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    const int j = lane + 64 * i;
                    if (j < nv) *(vec_t *)(A.dub + n * D + VEC * j) = (h[i] - y[i] * dots[wave][kk[i]]) * rk[i];
                }
                wave_lds_sync();   // the next position overwrites parts
            }
        }
    }
    if (!A.part) return;   // uniform over the workgroup
    // the four waves in wave order
    const float st = wave_sum(acc_t), sb = wave_sum(acc_b);
    if (lane == 0) { red[wave][0] = st; red[wave][1] = sb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        A.part[2 * (int64_t)blockIdx.x] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
        A.part[2 * (int64_t)blockIdx.x + 1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    }
}

constexpr int kSxSumThreads = 256;
__global__ __launch_bounds__(kSxSumThreads) void split_x0_scalars_kernel(const float *__restrict__ part, int64_t nblk, float *__restrict__ ds_t,
                                                                         float *__restrict__ ds_b) {
    __shared__ float s[kSxSumThreads][2];
    const int tid = threadIdx.x;
    const int64_t per = (nblk + kSxSumThreads - 1) / kSxSumThreads;
    const int64_t lo = min(nblk, tid * per), hi = min(nblk, lo + per);
    float a = 0.f, b = 0.f;
    for (int64_t i = lo; i < hi; ++i) { a += part[2 * i]; b += part[2 * i + 1]; }
    s[tid][0] = a; s[tid][1] = b;
    __syncthreads();
    if (tid == 0) {
        a = 0.f; b = 0.f;
        for (int i = 0; i < kSxSumThreads; ++i) { a += s[i][0]; b += s[i][1]; }
        if (ds_t) *ds_t = a;
        if (ds_b) *ds_b = b;
    }
}

// ------------------------------------------------------------------------------------------ validation (no HIP call)

// everything that does not need the pointers: also what the size query runs
static int split_x0_check_shape(const MotSplitX0Desc *d, bool backward) {
    if (!d) return set_error(MOT_EINVAL, "split_x0: null descriptor");
    if (d->struct_size != sizeof(MotSplitX0Desc))
        return set_error(MOT_EINVAL, "split_x0: struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(MotSplitX0Desc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EUNSUPPORTED, "split_x0: dtype %d is not built (MOT_F32 or MOT_BF16)", d->dtype);
    if (d->reserved0) return set_error(MOT_EINVAL, "split_x0: reserved0 %u", d->reserved0);
    if (d->n_rows < 0 || d->tokens_per_row < 0) return set_error(MOT_ESHAPE, "split_x0: negative shape");
    if (int rc = check_id_source_shape("split_x0", id_source_of(*d), backward)) return rc;
    if (d->tok_rows <= 0 || d->byte_rows <= 0 || d->model_dim <= 0 || d->byte_dim <= 0)
        return set_error(MOT_ESHAPE, "split_x0: empty table (tok %lld x %d, byte %lld x %d)", (long long)d->tok_rows, d->model_dim, (long long)d->byte_rows,
                         d->byte_dim);
    const int vec = d->dtype == MOT_BF16 ? 8 : 4;
    if (d->byte_dim % vec) return set_error(MOT_EUNSUPPORTED, "split_x0: byte_dim %d must be a multiple of %d elements (16 bytes)", d->byte_dim, vec);
    if ((int64_t)d->bpt * d->byte_dim != d->model_dim)
        return set_error(MOT_EUNSUPPORTED, "split_x0: model_dim %d != bpt*byte_dim = %d*%d (x0b is the cat of the byte rows)", d->model_dim, d->bpt, d->byte_dim);
    if (d->model_dim > kSxMaxDim) return set_error(MOT_EUNSUPPORTED, "split_x0: model_dim %d above %d is not built", d->model_dim, kSxMaxDim);
    if (int rc = check_id_source_limits("split_x0", id_source_of(*d))) return rc;
    if (d->byte_rows > 0x7fffffffLL / d->byte_dim || d->tok_rows > 0x7fffffffLL)
        return set_error(MOT_ESHAPE, "split_x0: tables of %lld and %lld rows", (long long)d->tok_rows, (long long)d->byte_rows);
    return MOT_OK;
}

// forward workspace:  [byte rows' rms factors: byte_rows fp32]
// backward workspace: [the factors][scalar partials: 2 per 16 positions][token sums: order, canon, pieces][d a: N x D fp32][d u: slab x D fp32]
struct SxLayout { size_t rnorm, part, sums, da, dub, total; int64_t slab, nblk; };
static SxLayout split_x0_layout(const MotSplitX0Desc &d, bool backward) {
    const size_t N = (size_t)(d.n_rows * d.tokens_per_row), D = (size_t)d.model_dim;
    SxLayout L{};
    L.slab = (int64_t)(N < (size_t)kSxSlab ? N : (size_t)kSxSlab);
    L.nblk = (int64_t)((N + kSxBlockTok - 1) / kSxBlockTok);
    Arena ar;
    L.rnorm = ar.take((size_t)d.byte_rows * sizeof(float));
    if (backward) {
        L.part = ar.take((size_t)L.nblk * 2 * sizeof(float));
        // a table at or above the token order's limit takes no token-table gradient (refused where one is asked for)
        L.sums = ar.take(d.tok_rows < kSxOrderLimit ? token_sums_ws_bytes((int64_t)N, d.tok_rows, d.model_dim, d.dtype) : 0);
        L.da = ar.take(d.tok_rows < kSxOrderLimit ? N * D * sizeof(float) : 0);
        L.dub = ar.take((size_t)L.slab * D * sizeof(float));
    }
    L.total = ar.o;
    return L;
}

size_t split_x0_workspace_bytes(const MotSplitX0Desc *d, bool backward) {
    if (split_x0_check_shape(d, backward)) return 0;
    if (d->n_rows == 0 || d->tokens_per_row == 0) return 0;
    return split_x0_layout(*d, backward).total;
}

int split_x0_check(const MotSplitX0Desc *d, const MotSplitX0Grads *g, bool backward) {
    if (int rc = split_x0_check_shape(d, backward)) return rc;
    if (backward && (!g || g->struct_size != sizeof(MotSplitX0Grads)))
        return set_error(MOT_EINVAL, "split_x0_bwd: grads struct missing or struct_size mismatch");
    if (!backward && !d->out_x0t && !d->out_x0b && !d->out_x)
        return set_error(MOT_EUNSUPPORTED, "split_x0: out_x0t, out_x0b and out_x are all null: nothing to compute");
    if (backward && !g->grad_x0t && !g->grad_x0b && !g->grad_x)
        return set_error(MOT_EUNSUPPORTED, "split_x0_bwd: grad_x0t, grad_x0b and grad_x are all null: nothing to compute");
    if (backward && g->d_tok_table && d->tok_rows >= kSxOrderLimit)
        return set_error(MOT_EUNSUPPORTED, "split_x0_bwd: a token table of %lld rows (>= 2^21 - 1, the token order's limit) gets no gradient here",
                         (long long)d->tok_rows);
    if (!d->tokens) return set_error(MOT_EINVAL, "split_x0: tokens must be non-null");
    if (!d->tok_table || !d->byte_table) return set_error(MOT_EINVAL, "split_x0: null tok_table or byte_table");
    if (!d->scale_tok || !d->scale_byte) return set_error(MOT_EINVAL, "split_x0: null scale_tok or scale_byte (device pointers to one fp32 each)");
    uintptr_t align = (uintptr_t)d->tok_table | (uintptr_t)d->byte_table;
    if (!backward) align |= (uintptr_t)d->out_x0t | (uintptr_t)d->out_x0b | (uintptr_t)d->out_x;
    else align |= (uintptr_t)g->grad_x0t | (uintptr_t)g->grad_x0b | (uintptr_t)g->grad_x | (uintptr_t)g->d_tok_table | (uintptr_t)g->d_byte_table;
    if (align & 15) return set_error(MOT_EINVAL, "split_x0: tables, outputs and gradients must be 16-byte aligned");
    if (int rc = check_id_source_ptrs("split_x0", id_source_of(*d))) return rc;
    if (d->n_rows == 0 || d->tokens_per_row == 0) return MOT_OK;
    return check_workspace("split_x0", backward, d->workspace, d->workspace ? d->workspace_bytes : (size_t)0, split_x0_layout(*d, backward).total);
}

// ------------------------------------------------------------------------------------------ launches
template <typename T, int NCH, int U>
static int launch_sx_fwd(const SplitArgs &S, int64_t blocks, size_t lds, hipStream_t stream) {
    static std::atomic<uint64_t> lds_ok{0};   // per-device bits
    if (lds > 48 * 1024)
        if (int rc = ensure_max_dyn_lds((const void *)split_x0_fwd_kernel<T, NCH, U>, lds_ok, "split_x0_fwd_kernel")) return rc;
    hipLaunchKernelGGL((split_x0_fwd_kernel<T, NCH, U>), dim3((unsigned)blocks), dim3(kThreads), lds, stream, S);
    return check_launch("split_x0_fwd_kernel");
}

int launch_split_x0_fwd(const MotSplitX0Desc &d, hipStream_t stream) {
    const SxLayout L = split_x0_layout(d, false);
    const float eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    float *rnorm = (float *)((char *)d.workspace + L.rnorm);
    if (int rc = launch_rows_rnorm(d.byte_table, d.byte_rows, d.byte_dim, eps, rnorm, d.dtype, stream)) return rc;
    SplitArgs S{};
    MixArgs &A = S.M;
    fill_mix_ids(A, id_source_of(d));
    A.tok_table = (const float *)d.tok_table; A.tok_rows = d.tok_rows; A.Dt = d.model_dim;
    A.byte_table = (const float *)d.byte_table; A.byte_rows = d.byte_rows; A.Db = d.byte_dim;
    A.eps = eps; A.scale_tok = d.scale_tok; A.scale_byte = d.scale_byte; A.byte_rnorm = rnorm;
    S.x0t = d.out_x0t; S.x0b = d.out_x0b; S.x = d.out_x; S.Dm = d.model_dim;
    int64_t blocks;
    size_t lds;
    if (int rc = wave_geometry("split_x0", A, d.n_rows, blocks, lds)) return rc;
    // NCH = 16-byte chunks per lane; U keeps ~8 independent 16-byte row loads per lane in flight (a token and a byte chunk per token)
    if (d.dtype == MOT_BF16) {
        switch ((S.Dm / 8 + 63) / 64) {
            case 1: return launch_sx_fwd<__bf16, 1, 4>(S, blocks, lds, stream);
            case 2: return launch_sx_fwd<__bf16, 2, 2>(S, blocks, lds, stream);
            default: return launch_sx_fwd<__bf16, 4, 1>(S, blocks, lds, stream);
        }
    }
    switch ((S.Dm / 4 + 63) / 64) {
        case 1: return launch_sx_fwd<float, 1, 4>(S, blocks, lds, stream);
        case 2:
        case 3:
        case 4: return launch_sx_fwd<float, 4, 1>(S, blocks, lds, stream);
        default: return launch_sx_fwd<float, 8, 1>(S, blocks, lds, stream);
    }
}

int launch_split_x0_bwd(const MotSplitX0Desc &d, const MotSplitX0Grads &gr, hipStream_t stream) {
    const int64_t N = d.n_rows * d.tokens_per_row;
    const int D = d.model_dim, Db = d.byte_dim, bpt = d.bpt;
    const bool bf = d.dtype == MOT_BF16;
    const size_t esz = bf ? 2 : 4;
    const float eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    const bool want_scalars = gr.d_scale_tok || gr.d_scale_byte;
    if (!gr.d_tok_table && !gr.d_byte_table && !want_scalars) return MOT_OK;
    const SxLayout L = split_x0_layout(d, true);
    char *ws = (char *)d.workspace;
    float *rnorm = (float *)(ws + L.rnorm), *part = (float *)(ws + L.part), *da = (float *)(ws + L.da), *dub = (float *)(ws + L.dub);
    int rc;
    if ((rc = launch_rows_rnorm(d.byte_table, d.byte_rows, Db, eps, rnorm, d.dtype, stream))) return rc;
    for (int64_t r0 = 0; r0 < N; r0 += L.slab) {   // (the slab is a whole number of workgroups' positions)
        const int64_t n = N - r0 < L.slab ? N - r0 : L.slab;
        auto rows_of = [&](const void *g) { return g ? (const void *)((const char *)g + (size_t)r0 * D * esz) : nullptr; };
        SplitBwdArgs A{};
        A.tokens = d.tokens + r0; A.ids = d.ids + r0 * bpt;
        A.tok_table = d.tok_table; A.byte_table = d.byte_table; A.byte_rnorm = rnorm;
        A.g_t = rows_of(gr.grad_x0t); A.g_b = rows_of(gr.grad_x0b); A.g_x = rows_of(gr.grad_x);
        A.s_t = d.scale_tok; A.s_b = d.scale_byte;
        A.da = gr.d_tok_table ? da + r0 * D : nullptr;
        A.dub = gr.d_byte_table ? dub : nullptr;
        A.part = want_scalars ? part + 2 * (r0 / kSxBlockTok) : nullptr;
        A.n = n; A.tok_rows = (int)d.tok_rows; A.byte_rows = (int)d.byte_rows; A.bpt = bpt; A.Db = Db; A.D = D; A.eps = eps; A.status = d.status;
        const unsigned nb = (unsigned)((n + kSxBlockTok - 1) / kSxBlockTok);
        if (bf) {
            switch ((D / 8 + 63) / 64) {
                case 1: hipLaunchKernelGGL((split_x0_rows_kernel<__bf16, 1>), dim3(nb), dim3(kThreads), 0, stream, A); break;
                case 2: hipLaunchKernelGGL((split_x0_rows_kernel<__bf16, 2>), dim3(nb), dim3(kThreads), 0, stream, A); break;
                default: hipLaunchKernelGGL((split_x0_rows_kernel<__bf16, 4>), dim3(nb), dim3(kThreads), 0, stream, A); break;
            }
        } else {
            switch ((D / 4 + 63) / 64) {
                case 1: hipLaunchKernelGGL((split_x0_rows_kernel<float, 1>), dim3(nb), dim3(kThreads), 0, stream, A); break;
                case 2:
                case 3:
                case 4: hipLaunchKernelGGL((split_x0_rows_kernel<float, 4>), dim3(nb), dim3(kThreads), 0, stream, A); break;
                default: hipLaunchKernelGGL((split_x0_rows_kernel<float, 8>), dim3(nb), dim3(kThreads), 0, stream, A); break;
            }
        }
        if ((rc = check_launch("split_x0_rows_kernel"))) return rc;
        if (!gr.d_byte_table) continue;
        // d_byte += the slab's d u rows, as the gradient of an un-normed fp32 byte_cat
        MotByteCatDesc c{};
        c.struct_size = sizeof(MotByteCatDesc); c.dtype = MOT_F32; c.n_rows = 1; c.tokens_per_row = n; c.bpt = bpt; c.byte_dim = Db; c.n_out = 1;
        c.id_source = MOT_IDS_GIVEN; c.ids = A.ids; c.eps = eps; c.status = d.status;
        c.slot[0].table = d.byte_table; c.slot[0].rows = d.byte_rows; c.slot[0].norm = 0; c.slot[0].dtype = MOT_F32;
        MotByteCatGrads cg{};
        cg.struct_size = sizeof(MotByteCatGrads);
        cg.slot[0].grad_out = dub; cg.slot[0].d_table = gr.d_byte_table;
        if ((rc = launch_byte_cat_bwd(c, cg, stream))) return rc;
    }
    if (want_scalars) {
        hipLaunchKernelGGL(split_x0_scalars_kernel, dim3(1), dim3(kSxSumThreads), 0, stream, part, L.nblk, gr.d_scale_tok, gr.d_scale_byte);
        if ((rc = check_launch("split_x0_scalars_kernel"))) return rc;
    }
    if (gr.d_tok_table)
        if ((rc = launch_token_sums_f32(d.tokens, N, d.tok_rows, D, d.dtype, da, D, gr.d_tok_table, gr.token_order, true, ws + L.sums, d.status, stream))) return rc;
    return MOT_OK;
}

}  // namespace mot
