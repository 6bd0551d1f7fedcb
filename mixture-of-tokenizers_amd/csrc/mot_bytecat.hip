// mot_bytecat.hip -- the bytes-only front-end and the byte value embeddings of modded-nanogpt/runs/5_bytes-in_bytes-valemb.py:
//     x0   = norm(reshape_bytes(embed_bytes(byte_inputs)))                      :225-232, 314   (runs 4, 5, 6)
//     ve_j = reshape_bytes(value_embeds_bytes[j](byte_inputs))                  :248, 305       (runs 2, 5, 8)
// forward and backward, fp32 and bf16 (include/mot.h, MotByteCatDesc).  There is no token row: an output row is the token's bpt
// table rows side by side, model_dim = bpt * byte_dim columns, optionally rms-normalised, and up to four tables are indexed by
// the same id stream.
//
// Forward (byte_cat_fwd_kernel, ONE launch for all outputs): a wave owns a unit of 16 or 32 consecutive tokens of one row and
// runs the index phase of the fused front-end once (mot_wave.hpp: WaveIndexer / wave_ids_given, unchanged), which leaves the
// unit's ids in wave-private LDS; it then streams every output from them.  Lane l owns the 16-byte chunks l, l + 64, ... of a
// row; a chunk's byte slot and its offset inside the table row are per-lane constants; table rows come from L2 (4 x 458 x 64
// bf16 = 234 KB), rows leave with non-temporal 16-byte stores.  A row without a norm is stored as loaded (a copy, bit for bit);
// a normed row takes the six-step DPP wave reduction of the CONCAT kernel for its sum of squares.  Algorithmic bytes per token:
// 4 + 2 bpt read (ids from the token->byte table) or 8 bpt (ids given), once for all outputs; n_out * e * model_dim written.
//
// Backward: d_table_j[ids[n, k], :] += dcat_j[n, k * byte_dim ...], dcat = g, or s g - (s^3 (g . cat) / model_dim) cat behind a norm.
//   byte_cat_coef_kernel  normed slots only, one wave per token: the two row scalars a = s and b = s^3 (g . cat) / model_dim from
//                         the re-gathered row, 8 bytes per token in the workspace.
//   byte_cat_bwd_kernel   a workgroup owns one (slot, column slice of the table, share of the tokens): the slice of the table's
//                         gradient sits in its LDS as 64-bit fixed point (mot_backward.hip's scheme: scale per workgroup from a
//                         sample of its own gradient rows, integer LDS atomics, so the sum inside a workgroup does not depend on
//                         the order of the adds), terms that do not convert and rows without an LDS row take the exact global
//                         float atomic, and the slice is flushed once with float atomics.  No token order, no sort.
#include <type_traits>

#include "mot_wave.hpp"

namespace mot {

constexpr int kCatMaxDim = 2048;
constexpr int kCatSlots = MOT_BYTE_CAT_MAX_OUT;

struct CatArgs {
    MixArgs M;   // the id part (what WaveIndexer / wave_ids_given read); byte_rows = the largest table's
    const void *table[kCatSlots];
    void *out[kCatSlots];
    int rows[kCatSlots], norm[kCatSlots];
    int n_out, Dm;
};

template <typename T> struct CatRaw;
template <> struct CatRaw<float> {
    static __device__ __forceinline__ void store_nt(float *p, float4v r) { __builtin_nontemporal_store(r, (float4v *)p); }
};
template <> struct CatRaw<__bf16> {
    static __device__ __forceinline__ void store_nt(__bf16 *p, bf16x8v r) { __builtin_nontemporal_store(r, (bf16x8v *)p); }
};

// ------------------------------------------------------------------------------------------ forward
// NCH: 16-byte chunks per lane (covers Dm <= 64 * NCH * VEC).  U: tokens in flight per wave and output.
template <typename T, int NCH, int U>
__global__ __launch_bounds__(kThreads) void byte_cat_fwd_kernel(const CatArgs C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_wave[];
    typedef typename Elem<T>::vec vec_t;
    typedef typename Elem<T>::raw raw_t;
    constexpr int VEC = Elem<T>::kVec;
    const MixArgs &A = C.M;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit_id = (int64_t)blockIdx.x * kWaves + wave;
    if (unit_id >= A.n_units) return;   // no barrier anywhere below: a wave may leave on its own
    const int64_t row = unit_id / A.units_per_row;
    const int64_t u0 = (unit_id - row * A.units_per_row) * A.unit;
    const int ntok = (int)min((int64_t)A.unit, A.T - u0);
    const int stream_eb = (A.id_source == MOT_IDS_FROM_TTB && A.pull_dir != kPullNone) ? A.ttb_elem : 0;
    const WaveLds W = wave_lds_carve(lds_wave + (size_t)wave * A.wave_lds, A.unit, A.bpt, false, stream_eb);

    // ---- the unit's byte ids into wave-private LDS, once for every output
    auto from_ttb = [&](auto indexer) {
        indexer.tokens();
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
        wave_ids_given(A, W, row, u0, ntok);
    }

    // ---- streaming: column VEC * c of a row belongs to slot VEC * c / Db (reshape_bytes, runs/5_*.py:225-228)
    const int Dm = C.Dm, Db = A.Db, nchunk = Dm / VEC, sv = A.bpt | 1;
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
    const int64_t tok0 = row * A.T + u0;
    bool oor = false;
#pragma unroll
    for (int j = 0; j < kCatSlots; ++j) {
        if (j >= C.n_out) break;
        const T *tab = (const T *)C.table[j];
        T *obase = (T *)C.out[j] + tok0 * (int64_t)Dm;
        const uint32_t rows = (uint32_t)C.rows[j];
        const bool norm = C.norm[j] != 0;
        for (int tb = 0; tb < ntok; tb += U) {
            raw_t br[U][NCH];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = min(tb + u, ntok - 1);   // the tail re-reads the last token; its store is skipped
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    int id = W.ids[t * sv + slot[i]];
                    if ((uint32_t)id >= rows) { oor = true; id = 0; }   // a table shorter than the largest one
                    br[u][i] = Elem<T>::load_raw(tab + (int64_t)id * Db + within[i]);
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = tb + u;
                T *orow = obase + (int64_t)t * Dm;
                if (norm) {
                    vec_t x[NCH];
                    float ss = 0.f;
#pragma unroll
                    for (int i = 0; i < NCH; ++i) {
                        x[i] = Elem<T>::widen(br[u][i]);
                        float s = 0.f;
#pragma unroll
                        for (int e = 0; e < VEC; ++e) s += x[i][e] * x[i][e];
                        ss += act[i] ? s : 0.f;
                    }
                    const float r = rms_scale(wave_sum(ss), Dm, A.eps);
                    if (t < ntok) {
#pragma unroll
                        for (int i = 0; i < NCH; ++i)
                            if (act[i]) Elem<T>::storev_nt(orow + VEC * (lane + 64 * i), x[i] * r);
                    }
                } else if (t < ntok) {
#pragma unroll
                    for (int i = 0; i < NCH; ++i)
                        if (act[i]) CatRaw<T>::store_nt(orow + VEC * (lane + 64 * i), br[u][i]);
                }
            }
        }
    }
    if (oor && A.status) atomicOr(A.status, kStatusByteOor);
}

// ------------------------------------------------------------------------------------------ backward
struct CatBwdSlot {
    const void *g, *table;
    float *d;
    float *coef;        // [N][2]: a, b of every token (normed slots), else null
    int rows, cs, prow; // column-slice width, table rows with an LDS row
    int first;          // blockIdx.y of the slot's first column slice
};
struct CatBwdArgs {
    const int64_t *ids;
    int64_t N;
    int bpt, Db, Dm, nslot;
    int lds_sums;       // 64-bit words of the largest slot's slice: the sample word sits behind them
    float eps;
    uint32_t *status;
    unsigned long long *counters;   // optional [2]: non-zero gradient terms added, and those of them that took the exact global path
    CatBwdSlot s[kCatSlots];
};

constexpr int kCatBwdThreads = 1024, kCatBwdWaves = kCatBwdThreads / 64;   // 16 waves, 4 per SIMD; one workgroup per CU by LDS
constexpr size_t kCatLdsBudget = 144 * 1024;                              // of the 160 KiB: the privatised slice
constexpr int kCatMinSlice = 8;                                           // columns: a slice of a gradient row is >= 16 contiguous bytes per slot

// a = s = rsqrt(mean(cat^2) + eps), b = s^3 (g . cat) / Dm of every token, so that dcat = a g - b cat  (= s (g - x (g.x) / Dm), x = s cat)
template <typename T>
__global__ __launch_bounds__(kThreads) void byte_cat_coef_kernel(const T *__restrict__ g, const T *__restrict__ table, uint32_t rows,
                                                                 const int64_t *__restrict__ ids, int64_t n, int bpt, int Db, int Dm, float eps,
                                                                 float *__restrict__ coef) {
    typedef typename Elem<T>::vec vec_t;
    constexpr int VEC = Elem<T>::kVec, NCH = kCatMaxDim / VEC / 64;
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (r >= n) return;
    const int nv = Dm / VEC;
    float ss = 0.f, m = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int j = lane + 64 * i;
        if (j < nv) {
            const int k = (VEC * j) / Db, w = VEC * j - k * Db;
            int64_t id = ids[r * bpt + k];
            if ((uint64_t)id >= (uint64_t)rows) id = 0;   // (flagged by the scatter kernel)
            const vec_t c = Elem<T>::loadv(table + id * Db + w), gv = Elem<T>::loadv(g + r * Dm + VEC * j);
#pragma unroll
            for (int e = 0; e < VEC; ++e) { ss += c[e] * c[e]; m += gv[e] * c[e]; }
        }
    }
    const float s = rms_scale(wave_sum(ss), Dm, eps);
    m = wave_sum(m);
    if (lane == 0) {
        coef[2 * r] = s;
        coef[2 * r + 1] = s * s * s * m * (1.0f / (float)Dm);
    }
}

template <typename T>
__global__ __launch_bounds__(kCatBwdThreads) void byte_cat_bwd_kernel(const CatBwdArgs A) {
    extern __shared__ unsigned long long cat_q[];   // [prow * cs] sums, then one word for the sample's maximum (no static LDS: the dynamic limit is the whole 160 KiB)
    constexpr int P = sizeof(T) == 2 ? 2 : 1;   // elements per lane item: bf16 is read in pairs, one dword per lane
    constexpr int Q = 4;                        // items a lane has in flight
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    CatBwdSlot S = A.s[0];
#pragma unroll
    for (int j = 1; j < kCatSlots; ++j)
        if (j < A.nslot && (int)blockIdx.y >= A.s[j].first) S = A.s[j];
    const int cs = S.cs, c0 = ((int)blockIdx.y - S.first) * cs, Db = A.Db, bpt = A.bpt;
    const int nq = S.prow * cs;
    uint32_t *fx_bits = (uint32_t *)(cat_q + A.lds_sums);   // behind the largest slot's sums
    for (int i = tid; i < nq; i += kCatBwdThreads) cat_q[i] = 0ull;
    if (tid == 0) *fx_bits = 0u;
    const T *g = (const T *)S.g, *table = (const T *)S.table;
    const bool normed = S.coef != nullptr;
    const int64_t per = (A.N + gridDim.x - 1) / gridDim.x;
    const int64_t lo = min(A.N, (int64_t)blockIdx.x * per), hi = min(A.N, lo + per);
    const int ipr = cs / P, ni = bpt * ipr;   // items per slot, items per token
    const float inv = 1.0f / (float)ipr;
    auto item = [&](int e, int &k, int &c) {   // item e of a token: slot and column inside the slice
        k = __float2int_rd(((float)e + 0.5f) * inv);   // e / ipr, exact for e < 2^22
        c = (e - k * ipr) * P;
    };
    auto load = [&](const T *p, float (&v)[P]) {
        if constexpr (P == 2) {
            const uint32_t w = *(const uint32_t *)p;
            v[0] = __uint_as_float(w << 16);
            v[1] = __uint_as_float(w & 0xffff0000u);
        } else {
            v[0] = *p;
        }
    };
    __syncthreads();   // orders the zeroing above
    // fixed-point scale of this workgroup's sums: v * 2^fx_k with the largest |a g| of the waves' first tokens at 2^27, so that a
    // term converts through a 32-bit integer.  Terms outside [2^12, 2^31) after scaling -- up to 16x the sample's maximum, down to
    // 2^-15 of it -- non-finite terms and rows without an LDS row take the exact global float atomic.
    {
        float gmax = 0.f;
        const int64_t n = lo + wave;
        if (n < hi) {
            for (int e = lane; e < ni; e += 64) {
                int k, c;
                item(e, k, c);
                float v[P];
                load(g + n * A.Dm + k * Db + c0 + c, v);
#pragma unroll
                for (int p = 0; p < P; ++p) gmax = fmaxf(gmax, fabsf(v[p]));
            }
            gmax = wave_max(gmax) * (normed ? fabsf(S.coef[2 * n]) : 1.0f);
            if (lane == 0 && gmax > 0.f && gmax < INFINITY) atomicMax(fx_bits, __float_as_uint(gmax));
        }
    }
    __syncthreads();
    const float fx_m = __uint_as_float(*fx_bits);
    const int fx_k = fx_m > 0.f ? min(27 - ilogbf(fx_m), 100) : 0;
    const uint32_t fx_lo_bits = __float_as_uint(ldexpf(1.0f, 12 - fx_k));
    const uint32_t fx_span = fx_m > 0.f ? __float_as_uint(ldexpf(1.0f, 31 - fx_k)) - fx_lo_bits : 0u;   // no sample: everything takes the exact path
    bool oor = false;
    unsigned n_terms = 0, n_exact = 0;   // per lane: a share of 2^31 tokens x 32 items stays below 2^32 per lane only for the sizes one launch takes
    for (int64_t n = lo + wave; n < hi; n += kCatBwdWaves) {
        int idv = 0;
        if (lane < bpt) {
            const int64_t v = A.ids[n * bpt + lane];
            if ((uint64_t)v >= (uint64_t)(uint32_t)S.rows) oor = true; else idv = (int)v;
        }
        float a = 1.f, b = 0.f;
        if (normed) { a = S.coef[2 * n]; b = S.coef[2 * n + 1]; }
        const T *grow = g + n * A.Dm + c0;
        for (int e0 = 0; e0 < ni; e0 += 64 * Q) {
            float gv[Q][P], tv[Q][P];
            int idq[Q], cq[Q];
            bool ok[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int e = e0 + 64 * q + lane;
                ok[q] = e < ni;
                int k, c;
                item(ok[q] ? e : 0, k, c);
                cq[q] = c;
                idq[q] = __shfl(idv, k, 64);
#pragma unroll
                for (int p = 0; p < P; ++p) { gv[q][p] = 0.f; tv[q][p] = 0.f; }
                if (ok[q]) {
                    load(grow + k * Db + c, gv[q]);
                    if (normed) load(table + (int64_t)idq[q] * Db + c0 + c, tv[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                if (!ok[q]) continue;
                const bool priv = idq[q] < S.prow;
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const float v = normed ? a * gv[q][p] - b * tv[q][p] : gv[q][p];
                    const uint32_t bits = __float_as_uint(v);
                    if ((bits << 1) == 0u) continue;
                    ++n_terms;
                    if (priv && ((bits & 0x7fffffffu) - fx_lo_bits) < fx_span)
                        atomicAdd(cat_q + (idq[q] * cs + cq[q] + p), (unsigned long long)(long long)__float2int_rn(ldexpf(v, fx_k)));
                    else {
                        ++n_exact;
                        atomicAdd(S.d + ((int64_t)idq[q] * Db + c0 + cq[q] + p), v);
                    }
                }
            }
        }
    }
    if (oor && A.status) atomicOr(A.status, kStatusByteOor);
    if (A.counters) {   // a measurement aid: one pair of atomics per lane, only when the caller asks
        atomicAdd(A.counters, (unsigned long long)n_terms);
        if (n_exact) atomicAdd(A.counters + 1, (unsigned long long)n_exact);
    }
    __syncthreads();
    for (int i = tid; i < nq; i += kCatBwdThreads) {   // the one flush of this workgroup
        const long long q = (long long)cat_q[i];
        if (q == 0) continue;
        const int r = i / cs, c = i - r * cs;
        atomicAdd(S.d + ((int64_t)r * Db + c0 + c), (float)ldexp((double)q, -fx_k));
    }
}

// ------------------------------------------------------------------------------------------ validation (no HIP call)

// everything that does not need the pointers: also what the two size queries run
static int byte_cat_check_shape(const MotByteCatDesc *d, bool backward) {
    if (!d) return set_error(MOT_EINVAL, "byte_cat: null descriptor");
    if (d->struct_size != sizeof(MotByteCatDesc))
        return set_error(MOT_EINVAL, "byte_cat: struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(MotByteCatDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EINVAL, "byte_cat: bad dtype %d", d->dtype);
    if (d->reserved0) return set_error(MOT_EINVAL, "byte_cat: reserved0 %u", d->reserved0);
    if (d->n_out < 1 || d->n_out > MOT_BYTE_CAT_MAX_OUT) return set_error(MOT_EUNSUPPORTED, "byte_cat: n_out %d outside [1, %d]", d->n_out, MOT_BYTE_CAT_MAX_OUT);
    if (d->n_rows < 0 || d->tokens_per_row < 0) return set_error(MOT_ESHAPE, "byte_cat: negative shape");
    if (int rc = check_id_source_shape("byte_cat", id_source_of(*d), backward)) return rc;
    const int vec = d->dtype == MOT_BF16 ? 8 : 4;
    if (d->byte_dim <= 0 || (d->byte_dim % vec))
        return set_error(MOT_EUNSUPPORTED, "byte_cat: byte_dim %d must be a positive multiple of %d elements (16 bytes)", d->byte_dim, vec);
    const int64_t Dm = (int64_t)d->bpt * d->byte_dim;
    if (Dm > kCatMaxDim) return set_error(MOT_EUNSUPPORTED, "byte_cat: model_dim %lld = bpt*byte_dim above %d is not built", (long long)Dm, kCatMaxDim);
    for (int j = 0; j < d->n_out; ++j) {
        if (d->slot[j].dtype != d->dtype)
            return set_error(MOT_EINVAL, "byte_cat: slot %d has dtype %d, the descriptor %d (all tables share one dtype)", j, d->slot[j].dtype, d->dtype);
        if (d->slot[j].rows <= 0 || d->slot[j].rows > 0x7fffffffLL / d->byte_dim)
            return set_error(MOT_ESHAPE, "byte_cat: slot %d has a table of %lld rows", j, (long long)d->slot[j].rows);
    }
    if (int rc = check_id_source_limits("byte_cat", id_source_of(*d))) return rc;
    return MOT_OK;
}

size_t byte_cat_workspace_bytes(const MotByteCatDesc *d) {
    byte_cat_check_shape(d, false);   // records the refusal's message; 0 either way, so a null table or out changes nothing here
    return 0;
}

// backward workspace: [a, b] of every token for every normed slot
static size_t cat_coef_bytes(const MotByteCatDesc &d) { return up256((size_t)(d.n_rows * d.tokens_per_row) * 2 * sizeof(float)); }
size_t byte_cat_bwd_workspace_bytes(const MotByteCatDesc *d) {
    if (byte_cat_check_shape(d, true)) return 0;
    for (int j = 0; j < d->n_out; ++j)   // the pointer the backward refuses (`out` is not read by it)
        if (!d->slot[j].table) { set_error(MOT_EINVAL, "byte_cat: slot %d has a null table", j); return 0; }
    size_t n = 0;
    for (int j = 0; j < d->n_out; ++j) n += d->slot[j].norm ? cat_coef_bytes(*d) : 0;
    return n;
}

int byte_cat_check(const MotByteCatDesc *d, const MotByteCatGrads *g, bool backward) {
    if (int rc = byte_cat_check_shape(d, backward)) return rc;
    if (backward && (!g || g->struct_size != sizeof(MotByteCatGrads)))
        return set_error(MOT_EINVAL, "byte_cat_bwd: grads struct missing or struct_size mismatch");
    for (int j = 0; j < d->n_out; ++j) {
        if (!d->slot[j].table) return set_error(MOT_EINVAL, "byte_cat: slot %d has a null table", j);
        if (!backward && !d->slot[j].out) return set_error(MOT_EINVAL, "byte_cat: slot %d has a null out", j);
        if (backward && g->slot[j].grad_out && !g->slot[j].d_table) return set_error(MOT_EINVAL, "byte_cat_bwd: slot %d has a grad_out but a null d_table", j);
    }
    // (the only front-end that reads `tokens` for the ids alone: it has no token table)
    if (d->id_source == MOT_IDS_FROM_TTB && (!d->tokens || !d->ttb)) return set_error(MOT_EINVAL, "byte_cat: tokens / ttb missing");
    if (int rc = check_id_source_ptrs("byte_cat", id_source_of(*d))) return rc;
    if (d->n_rows == 0 || d->tokens_per_row == 0 || !backward) return MOT_OK;
    return check_workspace("byte_cat", true, d->workspace, d->workspace_bytes, byte_cat_bwd_workspace_bytes(d));
}

// ------------------------------------------------------------------------------------------ launches
template <typename T, int NCH, int U>
static int launch_cat_fwd(const CatArgs &C, int64_t blocks, size_t lds, hipStream_t stream) {
    static std::atomic<uint64_t> lds_ok{0};   // per-device bits
    if (lds > 48 * 1024)
        if (int rc = ensure_max_dyn_lds((const void *)byte_cat_fwd_kernel<T, NCH, U>, lds_ok, "byte_cat_fwd_kernel")) return rc;
    hipLaunchKernelGGL((byte_cat_fwd_kernel<T, NCH, U>), dim3((unsigned)blocks), dim3(kThreads), lds, stream, C);
    return check_launch("byte_cat_fwd_kernel");
}

int launch_byte_cat_fwd(const MotByteCatDesc &d, hipStream_t stream) {
    CatArgs C{};
    MixArgs &A = C.M;
    fill_mix_ids(A, id_source_of(d));
    A.Db = d.byte_dim;
    A.eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    int64_t max_rows = 0;
    for (int j = 0; j < d.n_out; ++j) {
        C.table[j] = d.slot[j].table; C.out[j] = d.slot[j].out; C.rows[j] = (int)d.slot[j].rows; C.norm[j] = d.slot[j].norm;
        if (d.slot[j].rows > max_rows) max_rows = d.slot[j].rows;
    }
    A.byte_rows = max_rows;   // the index phase clamps to the largest table; the streaming loop clamps per table
    C.n_out = d.n_out; C.Dm = d.bpt * d.byte_dim;
    int64_t blocks;
    size_t lds;
    if (int rc = wave_geometry("byte_cat", A, d.n_rows, blocks, lds)) return rc;
    // NCH = 16-byte chunks per lane; U keeps ~8 independent 16-byte loads per lane in flight
    if (d.dtype == MOT_BF16) {
        switch ((C.Dm / 8 + 63) / 64) {
            case 1: return launch_cat_fwd<__bf16, 1, 4>(C, blocks, lds, stream);
            case 2: return launch_cat_fwd<__bf16, 2, 4>(C, blocks, lds, stream);
            case 3:
            default: return launch_cat_fwd<__bf16, 4, 2>(C, blocks, lds, stream);
        }
    }
    switch ((C.Dm / 4 + 63) / 64) {
        case 1: return launch_cat_fwd<float, 1, 4>(C, blocks, lds, stream);
        case 2: return launch_cat_fwd<float, 2, 4>(C, blocks, lds, stream);
        case 3:
        case 4: return launch_cat_fwd<float, 4, 2>(C, blocks, lds, stream);
        default: return launch_cat_fwd<float, 8, 1>(C, blocks, lds, stream);
    }
}

int launch_byte_cat_bwd(const MotByteCatDesc &d, const MotByteCatGrads &gr, hipStream_t stream) {
    const int64_t N = d.n_rows * d.tokens_per_row;
    const int Db = d.byte_dim, Dm = d.bpt * Db;
    const bool bf = d.dtype == MOT_BF16;
    const float eps = d.eps > 0.f ? d.eps : FLT_EPSILON;
    CatBwdArgs A{};
    A.ids = d.ids; A.N = N; A.bpt = d.bpt; A.Db = Db; A.Dm = Dm; A.eps = eps; A.status = d.status; A.counters = (unsigned long long *)d.counters;
    char *ws = (char *)d.workspace;
    size_t ws_at = 0, lds = 0;
    int slices = 0;
    for (int j = 0; j < d.n_out; ++j) {
        float *coef = nullptr;
        if (d.slot[j].norm) { coef = (float *)(ws + ws_at); ws_at += cat_coef_bytes(d); }   // the layout byte_cat_bwd_workspace_bytes sized
        if (!gr.slot[j].grad_out) continue;
        CatBwdSlot &S = A.s[A.nslot++];
        S.g = gr.slot[j].grad_out; S.table = d.slot[j].table; S.d = (float *)gr.slot[j].d_table; S.coef = coef; S.rows = (int)d.slot[j].rows;
        // the column slice: the whole row if the table's 64-bit sums fit the LDS, else halves of it (whole multiples of 4 columns, at
        // least kCatMinSlice); what still does not fit keeps the leading rows in LDS and sends the others down the exact path
        int cs = Db;
        while ((size_t)S.rows * cs * 8 > kCatLdsBudget && cs % 8 == 0 && cs / 2 >= kCatMinSlice) cs /= 2;
        S.cs = cs;
        S.prow = (int)std::min<size_t>((size_t)S.rows, kCatLdsBudget / ((size_t)cs * 8));
        S.first = slices;
        slices += Db / cs;
        lds = std::max(lds, (size_t)S.prow * cs * 8);
        if (coef) {
            const unsigned nb = (unsigned)((N + kWaves - 1) / kWaves);
            if (bf)
                hipLaunchKernelGGL(byte_cat_coef_kernel<__bf16>, dim3(nb), dim3(kThreads), 0, stream, (const __bf16 *)S.g, (const __bf16 *)S.table, (uint32_t)S.rows,
                                   d.ids, N, d.bpt, Db, Dm, eps, coef);
            else
                hipLaunchKernelGGL(byte_cat_coef_kernel<float>, dim3(nb), dim3(kThreads), 0, stream, (const float *)S.g, (const float *)S.table, (uint32_t)S.rows,
                                   d.ids, N, d.bpt, Db, Dm, eps, coef);
            if (int rc = check_launch("byte_cat_coef_kernel")) return rc;
        }
    }
    if (!A.nslot) return MOT_OK;
    A.lds_sums = (int)(lds / 8);
    lds += 8;
    // one workgroup per CU (the slice takes most of the LDS): the token shares fill the device's CUs once, so that every workgroup
    // zeroes and flushes its slice once per launch; a share is at least 64 tokens (four per wave: below that the zeroing and the
    // flush of up to 18 K sums outweigh the adds)
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
        return set_error(MOT_EHIP, "byte_cat_bwd: cannot read the device's compute-unit count");
    int64_t parts = std::max<int64_t>(1, cus / slices);
    parts = std::max<int64_t>(1, std::min<int64_t>(parts, N / 64));
    static std::atomic<uint64_t> lds_ok16{0}, lds_ok32{0};
    if (bf) {
        if (int rc = ensure_max_dyn_lds((const void *)byte_cat_bwd_kernel<__bf16>, lds_ok16, "byte_cat_bwd_kernel")) return rc;
        hipLaunchKernelGGL(byte_cat_bwd_kernel<__bf16>, dim3((unsigned)parts, (unsigned)slices), dim3(kCatBwdThreads), lds, stream, A);
    } else {
        if (int rc = ensure_max_dyn_lds((const void *)byte_cat_bwd_kernel<float>, lds_ok32, "byte_cat_bwd_kernel")) return rc;
        hipLaunchKernelGGL(byte_cat_bwd_kernel<float>, dim3((unsigned)parts, (unsigned)slices), dim3(kCatBwdThreads), lds, stream, A);
    }
    return check_launch("byte_cat_bwd_kernel");
}

}  // namespace mot
