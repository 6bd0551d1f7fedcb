// mot_values.hip -- token value embeddings: one to four tables of equal shape indexed by one token stream,
//     ve = [value_embed(toks_in) for value_embed in self.value_embeds]      scaled-pre-train/train_gpt.py:566, 600
//                                                                           modded-nanogpt/runs/71_*_toks-valemb.py:247, 303
// forward and backward, fp32 and bf16 (include/mot.h, MotValueEmbedsDesc).
//
// Forward (value_embeds_fwd_kernel, ONE launch for all tables): a wave owns 8 or 16 consecutive positions, reads their ids once
// (one lane each, clamped and flagged there) and streams every table's rows from them.  Lane l owns the 16-byte chunks l, l + 64,
// ... of a row; rows are stored as loaded (a copy, bit for bit) with non-temporal stores.  Algorithmic bytes per position:
// 4 + n * 2 * dim * e.
//
// Backward: d_table_j[r, :] = round(sum of grad_out_j[n, :] over the positions n with tokens[n] == r), written once.  It walks the
// token order of mot_group.hip (counts, starts, pos_sorted, id_sorted), whose groups are complete but hold their positions in an
// order that depends on the scheduling of the sort's atomics.
//   ve_canon_kernel,      put every group into ascending position order, the one order that does not depend on the run: a group
//   ve_canon_sort_kernel  of up to 64 positions by counting the smaller ones (one thread per sorted slot), a longer one by a
//                         bitonic sort in LDS (a workgroup per group), one of more than 32 768 positions by counting, a wave at a time.
//   ve_bwd_slices_kernel  the sorted stream is cut into slices of 64 slots; a wave owns one (slice, table, 64 chunks of columns)
//                         and walks its slots in order, one 16-byte chunk per lane, fp32 sums.  A group that lies inside the slice is
//                         rounded and stored; a piece of a group that crosses a slice boundary goes to the workspace in fp32: slot
//                         `head` of the slice when the group began in an earlier slice, slot `tail` otherwise.
//   ve_bwd_rows_kernel    a workgroup owns 16 ids of one (table, 64 chunks of columns): rows of absent ids are stored as +0; a group
//                         that crossed a boundary is the sum of its pieces in ascending slice order, four waves taking a quarter
//                         each and wave 0 adding the four results in wave order.  A hot id (3 % of a FineWeb batch) is thus spread
//                         over count / 64 waves in the slices kernel and over four here.
// No atomics on gradient elements, no memset, nothing for the caller to zero: every piece of the workspace that is read was
// written by the same call.
#include "mot_mix.hpp"

namespace mot {

constexpr int kVeMaxDim = 2048;
constexpr int kVeTables = MOT_VALUE_EMBEDS_MAX_TABLES;
constexpr int kVeSlice = 64;      // sorted slots per wave of the slices kernel
constexpr int kVeRowIds = 16;     // ids per workgroup of the rows kernel

// ------------------------------------------------------------------------------------------ forward
struct VeFwdArgs {
    const int32_t *tokens;
    int64_t N;
    int rows, D, n, unit;
    const void *table[kVeTables];
    void *out[kVeTables];
    uint32_t *status;
};

template <typename T> struct VeRaw;
template <> struct VeRaw<float> {
    static __device__ __forceinline__ void store_nt(float *p, float4v r) { __builtin_nontemporal_store(r, (float4v *)p); }
};
template <> struct VeRaw<__bf16> {
    static __device__ __forceinline__ void store_nt(__bf16 *p, bf16x8v r) { __builtin_nontemporal_store(r, (bf16x8v *)p); }
};

// NCH: 16-byte chunks per lane (covers D <= 64 * NCH * VEC).  U: positions in flight per wave.
template <typename T, int NCH, int U>
__global__ __launch_bounds__(kThreads) void value_embeds_fwd_kernel(const VeFwdArgs A) {
    typedef typename Elem<T>::raw raw_t;
    constexpr int VEC = Elem<T>::kVec;
    const int lane = threadIdx.x & 63;
    const int64_t p0 = ((int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6)) * A.unit;
    if (p0 >= A.N) return;   // no barrier below: a wave may leave on its own
    const int ntok = (int)min((int64_t)A.unit, A.N - p0);
    int id = 0;
    if (lane < ntok) {
        id = A.tokens[p0 + lane];
        if ((uint32_t)id >= (uint32_t)A.rows) { if (A.status) atomicOr(A.status, kStatusTokenOor); id = 0; }
    }
    const int D = A.D, nchunk = D / VEC;
    bool act[NCH];
#pragma unroll
    for (int i = 0; i < NCH; ++i) act[i] = lane + 64 * i < nchunk;
#pragma unroll
    for (int j = 0; j < kVeTables; ++j) {
        if (j >= A.n) break;
        const T *tab = (const T *)A.table[j] + VEC * lane;
        T *obase = (T *)A.out[j] + p0 * (int64_t)D + VEC * lane;
        for (int tb = 0; tb < ntok; tb += U) {
            raw_t br[U][NCH];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t r = __shfl(id, min(tb + u, ntok - 1));   // the tail re-reads the last position; its store is skipped
#pragma unroll
                for (int i = 0; i < NCH; ++i)
                    if (act[i]) br[u][i] = Elem<T>::load_raw(tab + r * D + VEC * 64 * i);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (tb + u >= ntok) break;
#pragma unroll
                for (int i = 0; i < NCH; ++i)
                    if (act[i]) VeRaw<T>::store_nt(obase + (int64_t)(tb + u) * D + VEC * 64 * i, br[u][i]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------ backward
struct VeBwdArgs {
    const int32_t *counts, *starts, *pos_sorted, *id_sorted;   // the token order (mot_group.hip)
    int32_t *canon;    // [N] the positions, every group ascending
    float *part;       // [slices][2: head, tail][nslot][D] fp32 pieces of the groups that cross a slice boundary
    int64_t N;
    int rows, D, nslot, nck;   // nck: blocks of 64 16-byte chunks per row
    int g_ld;                  // elements between the rows of g (D for the value embeddings' own gradients)
    const void *g[kVeTables];
    void *d[kVeTables];
};

__device__ __forceinline__ int ve_row(int id, int rows) { return (uint32_t)id < (uint32_t)rows ? id : 0; }
__device__ __forceinline__ int ve_pos(int p, int64_t N) { return (int)min((int64_t)max(p, 0), N - 1); }
// a group's [start, start + count) as the order states it, or an empty one if that does not lie inside [0, N): an order that was
// made for other tokens must not send a store out of bounds
__device__ __forceinline__ bool ve_group(const VeBwdArgs &A, int id, int &s, int &c) {
    s = A.starts[id];
    c = A.counts[id];
    return s >= 0 && c >= 0 && (int64_t)s + c <= A.N;
}

// ---- the canonical order: every group ascending by position.  Three ways by the group's size c:
//   c <= kVeSmall                  the slot's own thread counts the smaller positions of its group (at most 64 loads from L2);
//   kVeSmall < c <= cap            ve_canon_sort_kernel sorts the group in LDS (cap = what the LDS holds, at most 32 768 positions);
//   c > cap                        a wave counts for its 64 slots together: 64 positions of the group per load, handed round by lane.
//                                  Quadratic in c, so only for a batch where one id takes more than 32 768 positions.
constexpr int kVeSmall = 64, kVeSortMax = 32768, kVeSortThreads = 1024, kVeSortBlocks = 256;

__device__ __forceinline__ int ve_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int ve_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(kThreads) void ve_canon_kernel(const VeBwdArgs A, int cap) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool live = i < A.N;
    int p = 0, s = 0, c = 0;
    bool ok = false;
    if (live) {
        const int id = ve_row(A.id_sorted[i], A.rows);
        p = ve_pos(A.pos_sorted[i], A.N);
        ok = ve_group(A, id, s, c) && i >= s && i < (int64_t)s + c;
        if (!ok) A.canon[i] = p;   // an order that does not describe these tokens: keep the slot in bounds
    }
    if (ok && c <= kVeSmall) {
        int r = 0;
        const int32_t *q = A.pos_sorted + s;
        for (int j = 0; j < c; ++j) r += q[j] < p ? 1 : 0;
        A.canon[s + min(r, c - 1)] = p;
    }
    const bool big = ok && c > cap;
    if (__ballot(big) == 0) return;   // wave-uniform
    const int lo = ve_wave_min(big ? s : 0x7fffffff), hi = ve_wave_max(big ? s + c : 0);
    int r = 0;
    for (int base = lo; base < hi; base += 64) {
        const int j = base + lane;
        const int q = j < hi ? A.pos_sorted[j] : 0x7fffffff;
#pragma unroll
        for (int u = 0; u < 64; ++u) {
            const int qu = __builtin_amdgcn_readlane(q, u);
            r += (base + u >= s && base + u < s + c && qu < p) ? 1 : 0;
        }
    }
    if (big) A.canon[s + min(r, c - 1)] = p;
}

// Workgroup b looks at the ids b, b + gridDim.x, ... (hot ids are neighbours in a FineWeb batch: the stride spreads them) and
// sorts the positions of every group with kVeSmall < c <= cap in LDS, bitonic, padded with INT_MAX to a power of two.
__global__ __launch_bounds__(kVeSortThreads) void ve_canon_sort_kernel(const VeBwdArgs A, int cap) {
    extern __shared__ int32_t ve_key[];   // [cap] keys, [kVeSortThreads] ids to sort, their number: all dynamic, so that the raised limit holds all of it
    int32_t *list = ve_key + cap;
    int &nlist = list[kVeSortThreads];
    const int tid = threadIdx.x;
    for (int64_t r0 = 0; r0 < A.rows; r0 += (int64_t)kVeSortThreads * gridDim.x) {
        if (tid == 0) nlist = 0;
        __syncthreads();
        const int64_t id = r0 + (int64_t)tid * gridDim.x + blockIdx.x;
        if (id < A.rows) {
            int s, c;
            if (ve_group(A, (int)id, s, c) && c > kVeSmall && c <= cap) list[atomicAdd(&nlist, 1)] = (int)id;
        }
        __syncthreads();
        const int nl = nlist;
        for (int k = 0; k < nl; ++k) {   // in whatever order the list came out: the groups do not depend on one another
            const int s = A.starts[list[k]], c = A.counts[list[k]];
            int n2 = 2 * kVeSmall;
            while (n2 < c) n2 <<= 1;
            for (int i = tid; i < n2; i += kVeSortThreads) ve_key[i] = i < c ? A.pos_sorted[s + i] : 0x7fffffff;
            __syncthreads();
            for (int kk = 2; kk <= n2; kk <<= 1)
                for (int j = kk >> 1; j > 0; j >>= 1) {
                    for (int q = tid; q < n2 / 2; q += kVeSortThreads) {
                        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), ixj = i | j;
                        const int32_t x = ve_key[i], y = ve_key[ixj];
                        if ((x > y) == ((i & kk) == 0)) { ve_key[i] = y; ve_key[ixj] = x; }
                    }
                    __syncthreads();
                }
            for (int i = tid; i < c; i += kVeSortThreads) A.canon[s + i] = ve_key[i];
            __syncthreads();
        }
    }
}

// how a lane's chunk of a gradient row arrives: in the tables' dtype (G == T), or as fp32 rows for bf16 tables (the value mix's du,
// mot_valuemix.hip: the sums then start from unrounded terms)
template <typename G, typename T> struct VeIn {
    typedef typename Elem<T>::raw raw;
    static __device__ __forceinline__ raw load(const G *p) { return Elem<T>::load_raw(p); }
    static __device__ __forceinline__ typename Elem<T>::vec widen(raw r) { return Elem<T>::widen(r); }
};
template <> struct VeIn<float, __bf16> {
    typedef float8v raw;
    static __device__ __forceinline__ raw load(const float *p) {
        const float4v a = *(const float4v *)p, b = *(const float4v *)(p + 4);
        return float8v{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    }
    static __device__ __forceinline__ float8v widen(raw r) { return r; }
};

template <typename G, typename T>
__global__ __launch_bounds__(kThreads) void ve_bwd_slices_kernel(const VeBwdArgs A) {
    typedef typename Elem<T>::vec vec_t;
    typedef typename VeIn<G, T>::raw raw_t;
    constexpr int VEC = Elem<T>::kVec, U = 8;   // rows in flight per lane, whatever the groups' lengths
    const int lane = threadIdx.x & 63;
    const int64_t slice = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const int64_t b = slice * kVeSlice;
    if (b >= A.N) return;   // no barrier below
    const int js = blockIdx.y / A.nck, ck = blockIdx.y - js * A.nck;
    const int D = A.D, col = VEC * (ck * 64 + lane);
    const bool act = col < D;
    const G *g = (const G *)A.g[js] + (act ? col : 0);
    T *dt = (T *)A.d[js] + col;
    const int n = (int)min((int64_t)kVeSlice, A.N - b);
    int myid = -1, myp = 0;
    if (lane < n) {
        myid = ve_row(A.id_sorted[b + lane], A.rows);
        myp = ve_pos(A.canon[b + lane], A.N);
    }
    const int before = b > 0 ? ve_row(A.id_sorted[b - 1], A.rows) : -1;
    const int after = b + n < A.N ? ve_row(A.id_sorted[b + n], A.rows) : -1;
    // bit t: slot t is the last one of its group's run in this slice (lanes past the slice hold -1, so slot n - 1 always is)
    const int next_id = __shfl_down(myid, 1);   // by every lane: a lane left out of the shuffle hands nothing to its neighbour
    const unsigned long long ends = __ballot(lane < n && (lane == 63 || next_id != myid));
    vec_t acc = {};
    int m = 0;   // the first slot of the current run
    for (int t0 = 0; t0 < n; t0 += U) {
        raw_t r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = VeIn<G, T>::load(g + (int64_t)__shfl(myp, min(t0 + u, n - 1)) * A.g_ld);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int t = t0 + u;
            if (t >= n) break;
            acc += VeIn<G, T>::widen(r[u]);
            if (!((ends >> t) & 1ull)) continue;
            const int id = __shfl(myid, t);
            const bool opens = m > 0 || id != before;        // the group's first position is in this slice
            const bool closes = t + 1 < n || id != after;    // and its last one
            if (act) {
                if (opens && closes) {
                    Elem<T>::storev_nt(dt + (int64_t)id * D, acc);
                } else {
                    float *p = A.part + (((int64_t)slice * 2 + (opens ? 1 : 0)) * A.nslot + js) * (int64_t)D + col;
                    *(vec_t *)p = acc;
                }
            }
            acc = vec_t{};
            m = t + 1;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void ve_bwd_rows_kernel(const VeBwdArgs A) {
    typedef typename Elem<T>::vec vec_t;
    constexpr int VEC = Elem<T>::kVec;
    __shared__ __attribute__((aligned(32))) float red[kWaves][64][VEC];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int js = blockIdx.y / A.nck, ck = blockIdx.y - js * A.nck;
    const int D = A.D, col = VEC * (ck * 64 + lane);
    const bool act = col < D;
    T *dt = (T *)A.d[js] + col;
    const int id0 = blockIdx.x * kVeRowIds;
    // lane q < kVeRowIds of every wave reads group q of the workgroup's ids: one round trip for all of them
    int s = 0, c = 0;
    bool ok = false;
    if (lane < kVeRowIds && id0 + lane < A.rows) ok = ve_group(A, id0 + lane, s, c);
    const bool in = lane < kVeRowIds && id0 + lane < A.rows;
    const unsigned absent = (unsigned)__ballot(in && (!ok || c <= 0));
    const unsigned crosses = (unsigned)__ballot(ok && c > 0 && s / kVeSlice != (s + c - 1) / kVeSlice);
    // rows of ids that do not occur: +0, one row chunk per wave at a time
    for (int q = wave; q < kVeRowIds; q += kWaves)
        if (((absent >> q) & 1u) && act) Elem<T>::storev_nt(dt + (int64_t)(id0 + q) * D, vec_t{});
    // groups that crossed a slice boundary: the pieces in ascending slice order, a quarter per wave, then the waves in order
    for (unsigned left = crosses; left; left &= left - 1) {   // uniform over the workgroup, and so is everything the barriers depend on
        const int q = __ffs(left) - 1;
        const int gs = __shfl(s, q), gc = __shfl(c, q);
        const int a = gs / kVeSlice, z = (gs + gc - 1) / kVeSlice;
        const int per = (z - a + 1 + kWaves - 1) / kWaves;
        const int k0 = a + wave * per, k1 = min(k0 + per, z + 1);
        vec_t acc = {};
        if (act) {
            const float *base = A.part + (int64_t)js * D + col;
            const int64_t step = (int64_t)A.nslot * D;
            auto piece = [&](int k) {   // head (0) when the group began before slice k, else tail (1)
                return *(const vec_t *)(base + ((int64_t)k * 2 + ((int64_t)k * kVeSlice > gs ? 0 : 1)) * step);
            };
            int k = k0;
            for (; k + 4 <= k1; k += 4) {
                vec_t r[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) r[u] = piece(k + u);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc += r[u];
            }
            for (; k < k1; ++k) acc += piece(k);
        }
        *(vec_t *)red[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && act) {
            vec_t sum = *(const vec_t *)red[0][lane];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) sum += *(const vec_t *)red[w][lane];
            Elem<T>::storev_nt(dt + (int64_t)(id0 + q) * D, sum);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ validation (no HIP call)

static int value_embeds_check_shape(const MotValueEmbedsDesc *d) {
    if (!d) return set_error(MOT_EINVAL, "value_embeds: null descriptor");
    if (d->struct_size != sizeof(MotValueEmbedsDesc))
        return set_error(MOT_EINVAL, "value_embeds: struct_size %u != %zu (ABI mismatch)", d->struct_size, sizeof(MotValueEmbedsDesc));
    if (d->dtype != MOT_F32 && d->dtype != MOT_BF16) return set_error(MOT_EINVAL, "value_embeds: bad dtype %d", d->dtype);
    if (d->n_tables < 1 || d->n_tables > kVeTables)
        return set_error(MOT_EUNSUPPORTED, "value_embeds: n_tables %d outside [1, %d]", d->n_tables, kVeTables);
    if (d->n_tokens < 0 || d->tok_rows < 1) return set_error(MOT_ESHAPE, "value_embeds: bad shape");
    const int vec = d->dtype == MOT_BF16 ? 8 : 4;
    if (d->dim <= 0 || (d->dim % vec))
        return set_error(MOT_EUNSUPPORTED, "value_embeds: dim %d must be a positive multiple of %d elements (16 bytes)", d->dim, vec);
    if (d->dim > kVeMaxDim) return set_error(MOT_EUNSUPPORTED, "value_embeds: dim %d above %d is not built", d->dim, kVeMaxDim);
    if (d->tok_rows >= (1 << 21) - 1)
        return set_error(MOT_EUNSUPPORTED, "value_embeds: %lld rows (>= 2^21 - 1, the token order's limit) are not built", (long long)d->tok_rows);
    if (d->n_tokens > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "value_embeds: n_tokens exceeds 2^31");
    return MOT_OK;
}

// backward workspace: [token order, unless the caller brings one][canon: N int32][pieces: slices x 2 x n_tables x dim fp32]
struct VeLayout { size_t order, canon, part, total; int64_t slices; };
static VeLayout value_embeds_layout(const MotValueEmbedsDesc &d) {
    VeLayout L{};
    L.slices = (d.n_tokens + kVeSlice - 1) / kVeSlice;
    L.order = 0;
    L.canon = L.order + up256(group_positions_ws_ints(d.n_tokens, d.tok_rows) * sizeof(int32_t));
    L.part = L.canon + up256((size_t)d.n_tokens * sizeof(int32_t));
    L.total = L.part + up256((size_t)L.slices * 2 * d.n_tables * d.dim * sizeof(float));
    return L;
}

size_t value_embeds_bwd_workspace_bytes(const MotValueEmbedsDesc *d) {
    if (value_embeds_check_shape(d)) return 0;
    return d->n_tokens ? value_embeds_layout(*d).total : 0;
}

int value_embeds_check(const MotValueEmbedsDesc *d, const MotValueEmbedsGrads *g, bool backward) {
    if (int rc = value_embeds_check_shape(d)) return rc;
    if (backward && (!g || g->struct_size != sizeof(MotValueEmbedsGrads)))
        return set_error(MOT_EINVAL, "value_embeds_bwd: grads struct missing or struct_size mismatch");
    if (!d->tokens && (d->n_tokens > 0 || !backward)) return set_error(MOT_EINVAL, "value_embeds: null tokens");
    for (int j = 0; j < d->n_tables; ++j) {
        if (!backward && (!d->tables[j] || !d->outs[j])) return set_error(MOT_EINVAL, "value_embeds: table %d has a null table or out", j);
        if (backward && g->grad_outs[j] && !g->d_tables[j]) return set_error(MOT_EINVAL, "value_embeds_bwd: table %d has a grad_out but a null d_table", j);
    }
    if (d->n_tokens == 0) return MOT_OK;
    if (backward) {
        const size_t need = value_embeds_layout(*d).total;
        if (!d->workspace || d->workspace_bytes < need || ((uintptr_t)d->workspace & 15))
            return set_error(MOT_EWORKSPACE, "value_embeds_bwd: needs %zu 16-byte aligned workspace bytes, got %zu", need, d->workspace_bytes);
    }
    return MOT_OK;
}

// ------------------------------------------------------------------------------------------ launches
template <typename T, int NCH, int U>
static int launch_ve_fwd(const VeFwdArgs &A, hipStream_t stream) {
    const int64_t waves = (A.N + A.unit - 1) / A.unit, blocks = (waves + kWaves - 1) / kWaves;
    hipLaunchKernelGGL((value_embeds_fwd_kernel<T, NCH, U>), dim3((unsigned)blocks), dim3(kThreads), 0, stream, A);
    return check_launch("value_embeds_fwd_kernel");
}

int launch_value_embeds_fwd(const MotValueEmbedsDesc &d, hipStream_t stream) {
    VeFwdArgs A{};
    A.tokens = d.tokens; A.N = d.n_tokens; A.rows = (int)d.tok_rows; A.D = d.dim; A.n = d.n_tables; A.status = d.status;
    A.unit = d.n_tokens >= 131072 ? 16 : 8;   // positions per wave: enough waves to fill the device at a 64 x 1024 step
    for (int j = 0; j < d.n_tables; ++j) { A.table[j] = d.tables[j]; A.out[j] = d.outs[j]; }
    // NCH = 16-byte chunks per lane; U keeps ~8 independent 16-byte loads per lane in flight
    if (d.dtype == MOT_BF16) {
        switch ((d.dim / 8 + 63) / 64) {
            case 1: return launch_ve_fwd<__bf16, 1, 8>(A, stream);
            case 2: return launch_ve_fwd<__bf16, 2, 4>(A, stream);
            default: return launch_ve_fwd<__bf16, 4, 2>(A, stream);
        }
    }
    switch ((d.dim / 4 + 63) / 64) {
        case 1: return launch_ve_fwd<float, 1, 8>(A, stream);
        case 2: return launch_ve_fwd<float, 2, 4>(A, stream);
        case 3:
        case 4: return launch_ve_fwd<float, 4, 2>(A, stream);
        default: return launch_ve_fwd<float, 8, 1>(A, stream);
    }
}

// the token order (the caller's, or one made at L.order) and the canonical positions at L.canon
static int ve_order_and_canon(VeBwdArgs &A, const VeLayout &L, const int32_t *tokens, const int32_t *order, char *ws, uint32_t *status, hipStream_t stream) {
    const int64_t N = A.N;
    if (!order) {
        const int32_t *pos, *ids;
        if (int rc = launch_group_positions(tokens, N, A.rows, (int32_t *)(ws + L.order), &pos, &ids, status, stream)) return rc;
        order = (const int32_t *)(ws + L.order);
    }
    const GroupedPositions G = grouped_positions_view(order, N, A.rows);
    A.counts = G.counts; A.starts = G.starts; A.pos_sorted = G.pos_sorted; A.id_sorted = G.id_sorted;
    A.canon = (int32_t *)(ws + L.canon);
    A.part = (float *)(ws + L.part);
    // what the sort kernel's LDS holds: the smallest power of two that takes any group of this batch, 32 768 positions at most
    int cap = 2 * kVeSmall;
    while (cap < kVeSortMax && cap < N) cap <<= 1;
    hipLaunchKernelGGL(ve_canon_kernel, dim3((unsigned)((N + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream, A, cap);
    if (N > kVeSmall) {
        static std::atomic<uint64_t> lds_ok{0};   // per-device bits
        const size_t lds = ((size_t)cap + kVeSortThreads + 1) * sizeof(int32_t);
        if (lds > 48 * 1024)
            if (int rc = ensure_max_dyn_lds((const void *)ve_canon_sort_kernel, lds_ok, "ve_canon_sort_kernel")) return rc;
        hipLaunchKernelGGL(ve_canon_sort_kernel, dim3(kVeSortBlocks), dim3(kVeSortThreads), lds, stream, A, cap);
    }
    return check_launch("value_embeds canon kernels");
}

template <typename G, typename T>
static int ve_launch_sums(const VeBwdArgs &A, int64_t slices, hipStream_t stream) {
    const dim3 sg((unsigned)((slices + kWaves - 1) / kWaves), (unsigned)(A.nslot * A.nck));
    const dim3 rg((unsigned)(((int64_t)A.rows + kVeRowIds - 1) / kVeRowIds), (unsigned)(A.nslot * A.nck));
    hipLaunchKernelGGL((ve_bwd_slices_kernel<G, T>), sg, dim3(kThreads), 0, stream, A);
    hipLaunchKernelGGL(ve_bwd_rows_kernel<T>, rg, dim3(kThreads), 0, stream, A);
    return check_launch("value_embeds backward kernels");
}

int launch_value_embeds_bwd(const MotValueEmbedsDesc &d, const MotValueEmbedsGrads &gr, hipStream_t stream) {
    const bool bf = d.dtype == MOT_BF16;
    VeBwdArgs A{};
    A.N = d.n_tokens; A.rows = (int)d.tok_rows; A.D = A.g_ld = d.dim;
    A.nck = (d.dim / (bf ? 8 : 4) + 63) / 64;
    for (int j = 0; j < d.n_tables; ++j) {
        if (!gr.grad_outs[j]) continue;
        A.g[A.nslot] = gr.grad_outs[j];
        A.d[A.nslot++] = gr.d_tables[j];
    }
    if (!A.nslot) return MOT_OK;
    const VeLayout L = value_embeds_layout(d);
    if (int rc = ve_order_and_canon(A, L, d.tokens, gr.token_order, (char *)d.workspace, d.status, stream)) return rc;
    return bf ? ve_launch_sums<__bf16, __bf16>(A, L.slices, stream) : ve_launch_sums<float, float>(A, L.slices, stream);
}

// ------------------------------------------------------------------------------------------ one table from fp32 rows (mot_valuemix.hip)
// The same order, canon, slices and rows kernels for ONE table of `dtype` whose gradient rows are fp32 with a row stride of g_ld
// (a column block of du = dy W): d_table[r, :] = round(sum over the positions of id r of g[n, 0:dim]), written once, +0 where absent.
// `prepare` makes the order (unless the caller brings one) and the canonical positions; a later slot of the same tokens passes
// false and reuses what the workspace holds.
static MotValueEmbedsDesc token_sums_desc(int64_t n, int64_t rows, int dim, int dtype) {
    MotValueEmbedsDesc d{};
    d.dtype = dtype; d.n_tokens = n; d.tok_rows = rows; d.dim = dim; d.n_tables = 1;
    return d;
}
size_t token_sums_ws_bytes(int64_t n, int64_t rows, int dim, int dtype) { return n ? value_embeds_layout(token_sums_desc(n, rows, dim, dtype)).total : 0; }
int launch_token_sums_f32(const int32_t *tokens, int64_t n, int64_t rows, int dim, int dtype, const float *g, int g_ld, void *d_table,
                          const int32_t *order, bool prepare, char *ws, uint32_t *status, hipStream_t stream) {
    const bool bf = dtype == MOT_BF16;
    const VeLayout L = value_embeds_layout(token_sums_desc(n, rows, dim, dtype));
    VeBwdArgs A{};
    A.N = n; A.rows = (int)rows; A.D = dim; A.g_ld = g_ld;
    A.nck = (dim / (bf ? 8 : 4) + 63) / 64;
    A.g[0] = g; A.d[0] = d_table; A.nslot = 1;
    if (prepare) {
        if (int rc = ve_order_and_canon(A, L, tokens, order, ws, status, stream)) return rc;
    } else {
        const GroupedPositions G = grouped_positions_view(order ? order : (const int32_t *)(ws + L.order), n, rows);
        A.counts = G.counts; A.starts = G.starts; A.pos_sorted = G.pos_sorted; A.id_sorted = G.id_sorted;
        A.canon = (int32_t *)(ws + L.canon);
        A.part = (float *)(ws + L.part);
    }
    return bf ? ve_launch_sums<float, __bf16>(A, L.slices, stream) : ve_launch_sums<float, float>(A, L.slices, stream);
}

// ------------------------------------------------------------------------------------------ the two ends for a caller's own slices kernel (mot_once.hip)
// The same workspace (token_sums_ws_bytes) for ONE table whose slice sums another unit forms: the order (unless the caller brings
// one) and the canonical positions in front, the closing rows kernel behind.  The pieces lie at V.part as ve_bwd_slices_kernel lays
// them out with one slot: [slice][2: head, tail][dim] fp32.
int launch_token_canon(const int32_t *tokens, int64_t n, int64_t rows, int dim, int dtype, const int32_t *order, char *ws, uint32_t *status,
                       hipStream_t stream, TokenSumsView *V) {
    const VeLayout L = value_embeds_layout(token_sums_desc(n, rows, dim, dtype));
    VeBwdArgs A{};
    A.N = n; A.rows = (int)rows; A.D = A.g_ld = dim; A.nslot = 1;
    if (int rc = ve_order_and_canon(A, L, tokens, order, ws, status, stream)) return rc;
    *V = TokenSumsView{A.counts, A.starts, A.pos_sorted, A.id_sorted, A.canon, A.part};
    return MOT_OK;
}

int launch_token_rows_close(const TokenSumsView &V, int64_t n, int64_t rows, int dim, int dtype, void *d_table, hipStream_t stream) {
    const bool bf = dtype == MOT_BF16;
    VeBwdArgs A{};
    A.counts = V.counts; A.starts = V.starts; A.pos_sorted = V.pos_sorted; A.id_sorted = V.id_sorted; A.canon = V.canon; A.part = V.part;
    A.N = n; A.rows = (int)rows; A.D = A.g_ld = dim; A.nslot = 1;
    A.nck = (dim / (bf ? 8 : 4) + 63) / 64;
    A.d[0] = d_table;
    const dim3 rg((unsigned)(((int64_t)A.rows + kVeRowIds - 1) / kVeRowIds), (unsigned)A.nck);
    if (bf) hipLaunchKernelGGL(ve_bwd_rows_kernel<__bf16>, rg, dim3(kThreads), 0, stream, A);
    else hipLaunchKernelGGL(ve_bwd_rows_kernel<float>, rg, dim3(kThreads), 0, stream, A);
    return check_launch("ve_bwd_rows_kernel");
}

}  // namespace mot
