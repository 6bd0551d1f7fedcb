// mot_backward.hip -- the table-gradient scatter of the fused front-end's backward: the four scatter kernels, the choice
// between them (run_scatter) and the entry launch_embed_mix_bwd (called by mot_capi.hip and the cross-attention backward
// of mot_attn.hip).  SUM, NOOP and CONCAT are whole here; CONCAT_LINEAR (mot_bwd_linear.hip) and MEAN (mot_bwd_mean.hip)
// compute their dense parts and come back through run_scatter (mot_bwd.hpp).  The counting sort is mot_group.hip.
// dL/dx -> dL/d{token table, byte table, learned scalars}, what autograd computes for
// norm(embed_tokens(tok) + concat_k embed_bytes(byte_k)) and its variants
// (modded-nanogpt/runs/71_*.py:227-230, 312-314; 71041: 311-313; 71081: 302-315;
//  scaled-pre-train/train_gpt.py:342-348 tokens-only mode), called from loss.backward()
// (train_gpt.py:1319; mathblations/main.py:304).
//
// Per token (one wave): re-gather the rows, recompute the forward scalars (rms factors), push the
// upstream gradient back through the norms
//     x = y*r, r = rsqrt(mean(y^2)+eps)   =>   dy = r*(g - x*mean(g*x))
// and scatter-add:
//   * token table: FineWeb-shaped ids are heavily skewed (the most frequent id takes ~3 % of all
//     positions), and thousands of float atomics on one row serialise (measured: 4.5 ms per 524 k
//     tokens, 28 % of the atomic ceiling).  So the positions are first counting-sorted by token id
//     (bwd_rank_kernel -> bwd_scan_kernel -> bwd_place_kernel, three small kernels); each wave then
//     walks a contiguous stretch of the SORTED positions, keeps the running gradient row of the current
//     token in registers and issues one atomic row-add per run of equal tokens.  Lane l owns elements
//     l, l+64, ... of the row, so every atomic wave-instruction covers 256 contiguous bytes (the shape
//     that runs at the chip-wide atomic rate); float4-per-lane would spread each instruction over 1 KiB.
//   * byte table (458 rows hit 8.4 M times per step): privatised in LDS per workgroup as 64-bit fixed
//     point (ds_add_u64; ds_add_f32 issues one lane at a time on gfx950), flushed once with contiguous
//     global float atomics.
// 512-thread workgroups, one per CU (the LDS copy of the byte-table gradient takes up to 150 KB).
// Byte ids are taken as given (the forward returns them), so no tile machinery here.
// Float atomics make the sums order-dependent in the last bits, like the reference's own GPU
// embedding backward; the parity tests state the tolerance they use against a float64 evaluation.
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "mot_bwd.hpp"

namespace mot {

// Ordering of one wave's traffic on its per-slot LDS accumulators (seg / segr / seg_q): a plain zeroing store by every lane,
// LDS atomics from other lanes, a plain read-back.  DS instructions of one wave execute in issue order; what has to be pinned is
// the COMPILER's order across lanes: a release fence, a wave barrier (lanes are separate threads to the memory model: the
// barrier is what orders lane A's store before lane B's atomic) and an acquire fence.  No instruction beyond the waits the
// fences imply.
__device__ __forceinline__ void seg_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

constexpr int kBwdThreads = 512;  // 8 waves, 2 per SIMD: a 256-register budget per lane
constexpr int kBwdWaves = kBwdThreads / 64;
constexpr int kWindow = 64;  // sorted positions per wave work item

// One launch of a scatter kernel: the kernel's dynamic-LDS limit is raised once per (instantiation, device), then `blocks`
// workgroups of `threads` go out, at most one per CU (the kernels are persistent: their waves stride over the sorted positions).
template <auto Kernel>
static int launch_scatter(const BwdArgs &A, size_t lds, hipStream_t stream, int threads, int64_t blocks, const char *name) {
    static std::atomic<uint64_t> lds_ok{0};   // per-device bits
    if (int rc_lds = ensure_max_dyn_lds((const void *)Kernel, lds_ok, name)) return rc_lds;
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(Kernel, dim3((unsigned)blocks), dim3(threads), lds, stream, A);
    return check_launch(name);
}

// element i of a float or bf16 array (uniform choice per launch)
__device__ __forceinline__ float ld_in(const float *base, int64_t i, int bf16) {
    return bf16 ? (float)((const __bf16 *)base)[i] : base[i];
}

template <int MODE, int NE>
__global__ __launch_bounds__(kBwdThreads) void embed_mix_bwd_kernel(const BwdArgs A) {
    extern __shared__ unsigned long long lds_q[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbyte = A.priv_rows * A.Db;
    unsigned long long *dbyte_q = lds_q;              // [priv_rows*Db] fixed-point sums (two's complement)
    float *lds_f = (float *)(lds_q + nbyte);
    float *seg = lds_f + wave * kMaxBpt;              // per-wave per-slot dot products
    float *segr = lds_f + (kBwdWaves + wave) * kMaxBpt;  // per-wave per-slot rms factor (two-id-tensor norm)
    uint32_t *fx_bits = (uint32_t *)(lds_f + 2 * kBwdWaves * kMaxBpt);  // max |v| over the waves' first tokens (float bits)
    for (int i = tid; i < nbyte; i += kBwdThreads) dbyte_q[i] = 0ull;
    if (tid == 0) *fx_bits = 0u;
    __syncthreads();
    // LDS float atomics run one lane at a time on gfx950 (ds_add_f32: ~190 cycles per wave-instruction, ds_add_u64: ~20,
    // tools/ubench/lds_atomic.hip), so the privatised sums are 64-bit fixed point: v * 2^fx_k, fx_k chosen per workgroup so
    // that the largest |v| of the waves' first tokens lands at 2^28.  Terms outside [2^12, 2^40) after scaling (too coarse /
    // too close to the 2^62 budget of <= 2^22 adds) and rows without a slot take the exact global float atomic instead,
    // so the result never depends on the choice of scale -- only the speed does.
    int fx_k = 0;
    bool fx_pending = MODE != MOT_MIX_NOOP;
    auto byte_slot = [&](int id) { return id < A.priv_lo ? id : (id >= A.priv_hi0 ? id - A.priv_hi0 + A.priv_lo : -1); };
    auto add_byte = [&](int id, int wi, float v) {
        const int sl = byte_slot(id);
        const float x = rintf(ldexpf(v, fx_k)), ax = fabsf(x);
        if (sl >= 0 && ax < 0x1p40f && (ax >= 0x1p12f || v == 0.f)) {
            if (v != 0.f) atomicAdd(dbyte_q + sl * A.Db + wi, (unsigned long long)(long long)x);
        } else {
            atomicAdd(A.d_byte + id * A.Db + wi, v);   // exact path (also carries inf / nan through)
        }
    };

    const int D = A.D;
    const float inv_db = MODE != MOT_MIX_NOOP ? 1.0f / (float)A.Db : 0.f;
    // element e = lane + 64*j of a row lives in byte slot e / Db; (e + 0.5) * (1/Db) floors exactly for e < 2048
    auto slot_of = [&](int eb) { return MODE != MOT_MIX_NOOP ? __float2int_rd(((float)eb + 0.5f) * inv_db) : 0; };
    const int Dt = A.Dt;
    auto tok_off = [&](int e) { const int o = e - A.tok_lo; return (e < D && (unsigned)o < (unsigned)Dt) ? o : -1; };
    auto byte_off = [&](int e) { const int o = e - A.byte_lo; return (MODE != MOT_MIX_NOOP && e < D && (unsigned)o < (unsigned)A.nbk) ? o : -1; };
    // norm over the sum of two embeddings only exists in front of the concat mixin (train_gpt.py:378, 443)
    const bool pair_norm = split_row(MODE) && A.norm_byte && A.ids_b;
    const float s_tok = A.scale_tok ? *A.scale_tok : 1.0f;
    const float s_byte = A.scale_byte ? *A.scale_byte : 1.0f;
    float ds_t = 0.f, ds_b = 0.f;

    float acc[NE];  // running d(token row) of the current run of equal tokens
    int cur = -1;
    auto flush = [&]() {
        if (cur < 0 || (A.abl & 2)) return;
        float *drow = A.d_tok + (int64_t)cur * Dt;
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int o = tok_off(lane + 64 * j);
            if (o >= 0) atomicAdd(drow + o, acc[j]);
        }
    };
    // Each position needs position -> token -> rows and position -> byte ids -> byte rows: up to four
    // dependent round trips.  The index side (position, token, byte ids) of position i+1 is therefore
    // fetched while position i's rows are in flight, leaving one row-fetch latency per position.
    auto load_ids = [&](int64_t n, int (&ids)[NE]) {
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            ids[j] = 0;
            const int eb = byte_off(lane + 64 * j);
            if (eb >= 0) {
                int64_t ia = A.ids_a[n * A.bpt + slot_of(eb)];
                if ((uint64_t)ia >= (uint64_t)A.byte_rows) { if (A.status) atomicOr(A.status, kStatusByteOor); ia = 0; }
                ids[j] = (int)ia;
            }
        }
    };
    auto load_tok = [&](int64_t n) {
        int t = A.tokens[n];
        if ((uint64_t)(uint32_t)t >= (uint64_t)A.tok_rows) {
            if (A.status && lane == 0) atomicOr(A.status, kStatusTokenOor);
            t = 0;
        }
        return t;
    };
    const int64_t nwin = (A.n_tokens + kWindow - 1) / kWindow;
    for (int64_t w = (int64_t)blockIdx.x * kBwdWaves + wave; w < nwin; w += (int64_t)gridDim.x * kBwdWaves) {
    const int64_t s_end = min(A.n_tokens, (w + 1) * kWindow);
    int64_t n_nx = A.pos_sorted[w * kWindow];
    int tok_nx = load_tok(n_nx);
    int id_nx[NE];
    load_ids(n_nx, id_nx);
    for (int64_t si = w * kWindow; si < s_end; ++si) {
        const int64_t n = n_nx;
        const int tok = tok_nx;
        int id1[NE];
#pragma unroll
        for (int j = 0; j < NE; ++j) id1[j] = id_nx[j];
        // index of the next position first (oldest outstanding load), then this position's rows
        const int64_t s_nx = min(si + 1, s_end - 1);
        n_nx = A.pos_sorted[s_nx];
        if (tok != cur) {
            flush();
            cur = tok;
#pragma unroll
            for (int j = 0; j < NE; ++j) acc[j] = 0.f;
        }
        const int64_t trow = (int64_t)tok * Dt, grow = n * (int64_t)(A.g_ld ? A.g_ld : D);   // (g_ld: gradient rows that are columns of a wider matrix)
        float an[NE], bn[NE], dy[NE];
        // ---- gather (the same rows the forward read)
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int e = lane + 64 * j;
            const int et = tok_off(e), eb = byte_off(e);
            an[j] = et >= 0 ? ld_in(A.tok_table, trow + et, A.in_bf16) : 0.f;
            dy[j] = e < D ? ld_in(A.grad_out, grow + e, A.in_bf16) : 0.f;  // holds g until the norm backward below
            bn[j] = 0.f;
            if (eb >= 0) {
                const int sl = slot_of(eb), wi = eb - sl * A.Db;
                float v = ld_in(A.byte_table, (int64_t)id1[j] * A.Db + wi, A.in_bf16);
                if (A.ids_b) {
                    int64_t ib = A.ids_b[n * A.bpt + sl];
                    if ((uint64_t)ib >= (uint64_t)A.byte_rows) { if (A.status) atomicOr(A.status, kStatusByteOor); ib = 0; }
                    v += ld_in(A.byte_table, ib * A.Db + wi, A.in_bf16);
                }
                if (A.norm_byte && !pair_norm) v *= A.byte_rnorm[id1[j]];
                bn[j] = v;  // normalised, unscaled
            }
        }
        if (pair_norm) {
            // norm(emb(padded) + emb(pulled)) (train_gpt.py:378): the rms factor belongs to the (token, slot) pair,
            // not to a table row -- reduce sum(b^2) per slot through the wave's LDS accumulators
            segr[lane] = 0.f;   // all 64 lanes (kMaxBpt entries): a `lane < bpt` guard lets the compiler reorder the adds around it
            seg_sync();
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const int eb = byte_off(lane + 64 * j);
                if (eb >= 0) atomicAdd(&segr[slot_of(eb)], bn[j] * bn[j]);
            }
            seg_sync();
            segr[lane] = rms_scale(segr[lane], A.Db, A.eps);
            seg_sync();
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const int eb = byte_off(lane + 64 * j);
                if (eb >= 0) bn[j] *= segr[slot_of(eb)];
            }
        }
        tok_nx = load_tok(n_nx);
        load_ids(n_nx, id_nx);
        // ---- forward scalars
        float ra = 1.f;
        if (A.norm_tok) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < NE; ++j) ss += an[j] * an[j];
            ra = rms_scale(wave_sum(ss), Dt, A.eps);
#pragma unroll
            for (int j = 0; j < NE; ++j) an[j] *= ra;
        }
        if (A.norm_out) {
            float ss = 0.f;
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const float y = an[j] * s_tok + (mixes_bytes(MODE) ? bn[j] * s_byte : 0.f);
                ss += y * y;
            }
            const float ry = rms_scale((A.abl & 4) ? ss : wave_sum(ss), D, A.eps);
            float m = 0.f;
#pragma unroll
            for (int j = 0; j < NE; ++j) m += dy[j] * ((an[j] * s_tok + (mixes_bytes(MODE) ? bn[j] * s_byte : 0.f)) * ry);
            m = ((A.abl & 4) ? m : wave_sum(m)) / (float)D;
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const float x = (an[j] * s_tok + (mixes_bytes(MODE) ? bn[j] * s_byte : 0.f)) * ry;
                dy[j] = ry * (dy[j] - x * m);
            }
        }
        // ---- token side
        {
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < NE; ++j) dot += dy[j] * an[j];
            ds_t += dot;  // d scale_tok = sum dy * a_n
            float mt = 0.f;
            if (A.norm_tok) mt = wave_sum(dot * s_tok) / (float)Dt;
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const float da = dy[j] * s_tok;
                acc[j] += A.norm_tok ? ra * (da - an[j] * mt) : da;
            }
        }
        // ---- byte side
        if (MODE != MOT_MIX_NOOP) {
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < NE; ++j) dot += dy[j] * bn[j];
            ds_b += dot;
            if (A.norm_byte) {  // per-slot mean(db * b_n): slots are ragged lane groups -> LDS accumulators
                seg[lane] = 0.f;
                seg_sync();
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const int eb = byte_off(lane + 64 * j);
                    if (eb >= 0) atomicAdd(&seg[slot_of(eb)], dy[j] * s_byte * bn[j]);
                }
                seg_sync();
            }
            float vmax = 0.f;
#pragma unroll
            for (int j = 0; j < NE; ++j) {   // dy[j] <- gradient w.r.t. the (un-normalised) byte-table element
                const int eb = byte_off(lane + 64 * j);
                if (eb < 0) continue;
                const int sl = slot_of(eb);
                const float db = dy[j] * s_byte;
                float v = db;
                if (A.norm_byte) v = (pair_norm ? segr[sl] : A.byte_rnorm[id1[j]]) * (db - bn[j] * (seg[sl] / (float)A.Db));
                dy[j] = v;
                vmax = fmaxf(vmax, fabsf(v));
            }
            if (fx_pending) {   // once per wave: agree on the workgroup's fixed-point scale
                vmax = wave_max(vmax);
                if (lane == 0 && vmax > 0.f && vmax < INFINITY) atomicMax(fx_bits, __float_as_uint(vmax));
                __syncthreads();
                const float m = __uint_as_float(*fx_bits);
                fx_k = m > 0.f ? 28 - ilogbf(m) : 0;
                fx_pending = false;
            }
#pragma unroll
            for (int j = 0; j < NE; ++j) {
                const int eb = byte_off(lane + 64 * j);
                if (eb < 0 || (A.abl & 1)) continue;
                const int sl = slot_of(eb), wi = eb - sl * A.Db;
                add_byte(id1[j], wi, dy[j]);
                if (A.ids_b) {
                    int64_t ib = A.ids_b[n * A.bpt + sl];
                    if ((uint64_t)ib >= (uint64_t)A.byte_rows) ib = 0;
                    add_byte((int)ib, wi, dy[j]);
                }
            }
            if (A.norm_byte) seg_sync();  // seg is rewritten by the next token
        }
    }
    }
    // ---- flush
    flush();
    if (A.d_scale_tok) { ds_t = wave_sum(ds_t); if (lane == 0) atomicAdd(A.d_scale_tok, ds_t); }
    if (MODE != MOT_MIX_NOOP && A.d_scale_byte) { ds_b = wave_sum(ds_b); if (lane == 0) atomicAdd(A.d_scale_byte, ds_b); }
    if (MODE != MOT_MIX_NOOP) {
        if (fx_pending) {   // a wave without work still meets the others at the scale barrier
            __syncthreads();
            const float m = __uint_as_float(*fx_bits);
            fx_k = m > 0.f ? 28 - ilogbf(m) : 0;
        }
        __syncthreads();
        for (int i = tid; i < nbyte; i += kBwdThreads) {
            const long long q = (long long)dbyte_q[i];
            if (q == 0) continue;
            const int sl = i / A.Db, wi = i - sl * A.Db;
            const int row = sl < A.priv_lo ? sl : sl - A.priv_lo + A.priv_hi0;
            atomicAdd(A.d_byte + row * A.Db + wi, (float)ldexp((double)q, -fx_k));
        }
    }
}

// ------------------------------------------------------------------------------------------
// Lean variant for the layouts where a row is "full": SUM / NOOP with D == 64 * NE (the headline shapes: 768, 1024,
// 2048, 256 ...) and the CONCAT_LINEAR scatter whose row splits into a token part and a byte part on 64-element
// boundaries.  Same algorithm as embed_mix_bwd_kernel, minus everything the general layout needs per element: the slot
// and within-slot index of a lane's elements are computed once, position and token id are wave-uniform scalars (rows
// are addressed as SGPR base + immediates), a token's byte ids are loaded once by lanes < bpt and handed out with
// ds_bpermute, the token row is read once per run of equal tokens, and the byte-table adds are straight-line 64-bit
// fixed-point LDS atomics.  ~5x fewer instructions per position than the general kernel.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long to_fixed(float v, int k) {
    // round(v * 2^k) as two's complement in 64 bits, |v * 2^k| < 2^51: add 1.5 * 2^52 and read the mantissa
    const double d = ldexp((double)v, k) + 6755399441055744.0;
    return (unsigned long long)(__double_as_longlong(d) - 0x4338000000000000ll);
}


template <int MODE, int NE, bool BF>   // BF: tables and grad_out are bf16 (SUM / NOOP; the CONCAT_LINEAR path widens its operands first)
__global__ __launch_bounds__(kBwdThreads) void embed_mix_bwd_full_kernel(const BwdArgs A) {
    constexpr int D = 64 * NE;
    extern __shared__ unsigned long long lds_q[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform for the compiler too: scalar loop control below
    const int nbyte = A.priv_rows * A.Db;
    unsigned long long *dbyte_q = lds_q;
    unsigned long long *seg_q = lds_q + nbyte + wave * kMaxBpt;                      // per-wave per-slot sums (byte-norm backward)
    uint32_t *fx_bits = (uint32_t *)(lds_q + nbyte + kBwdWaves * kMaxBpt);
    for (int i = tid; i < nbyte; i += kBwdThreads) dbyte_q[i] = 0ull;
    if (tid == 0) *fx_bits = 0u;
    // SPLIT: the gradient row is du of CONCAT_LINEAR -- [token part | byte part] (or the reverse), every 64-element
    // chunk j belonging wholly to one part (host-checked); SUM / NOOP rows are token part and byte part at once.
    constexpr bool SPLIT = split_row(MODE);
    constexpr bool BYTES = MODE != MOT_MIX_NOOP;
    uint32_t tmask = 0, bmask = 0;   // bit j: chunk j carries token-row / byte-row elements
#pragma unroll
    for (int j = 0; j < NE; ++j) {
        const int e0 = 64 * j;
        if (!SPLIT || (e0 >= A.tok_lo && e0 < A.tok_lo + A.Dt)) tmask |= 1u << j;
        if (MODE == MOT_MIX_SUM || (SPLIT && e0 >= A.byte_lo && e0 < A.byte_lo + A.nbk)) bmask |= 1u << j;
    }
    const bool dual = BYTES && A.ids_b != nullptr;
    const bool pair_norm = SPLIT && dual && A.norm_byte;   // norm(emb(padded) + emb(pulled)), train_gpt.py:378
    const float s_tok = A.scale_tok ? *A.scale_tok : 1.0f;
    const float s_byte = A.scale_byte ? *A.scale_byte : 1.0f;
    float ds_t = 0.f, ds_b = 0.f;
    // element lane + 64 j of a row: ds_bpermute address of its byte slot's lane (slot * 4) and byte offset of the element
    // within a byte-table row, for 4-byte elements (x2 in the 64-bit LDS copy, /2 for bf16 tables)
    // Register slot j of a lane holds row element lane + 64 j (fp32: one dword per lane per load), or, for bf16 rows,
    // 2 lane + 128 (j / 2) + (j % 2): a lane loads PAIRS of adjacent bf16 as one dword (2-byte lane loads run at a
    // fraction of the dword rate), and a pair shares its byte slot (Db is even, host-checked), so one ds_bpermute and one
    // dword gather serve both.
    auto elem = [&](int j) { return BF ? 2 * lane + 128 * (j >> 1) + (j & 1) : lane + 64 * j; };
    int sl4[NE], wi4[NE];
#pragma unroll
    for (int j = 0; j < NE; ++j) {
        const int eb = max(elem(j) - A.byte_lo, 0), sl = BYTES ? eb / A.Db : 0;
        sl4[j] = sl * 4;
        wi4[j] = (eb - sl * A.Db) * 4;
    }
    constexpr uint32_t esz = BF ? 2u : 4u;
    const uint32_t lane4 = (uint32_t)lane * 4u;   // byte offset of a lane's first dword in a row (one fp32 / two bf16 elements)
    const uint32_t row8 = (uint32_t)A.Db * 8u;
    // Rows are addressed as (wave-uniform base pointer) + (32-bit byte offset): the position and its token id are made
    // scalar with readfirstlane, so a row's 64-bit address lives in SGPRs and the per-element offsets are immediates.
    // A row is first requested RAW (kRaw dwords per lane: one fp32 element or two bf16 each) and turned into floats later,
    // after everything else the position needs has been requested too -- unpacking bf16 pairs right at the load makes the
    // compiler wait for the row before it issues the byte-row gathers.
    constexpr int kRaw = BF ? (NE + 1) / 2 : NE;   // (bf16 kernels are launched with even NE only)
    auto load_raw = [&](const char *rbase, uint32_t (&raw)[kRaw], uint32_t mask) {   // mask: 64-element chunks present (fp32 split rows)
#pragma unroll
        for (int g = 0; g < kRaw; ++g) raw[g] = (BF || (mask >> g & 1)) ? *(const uint32_t *)(rbase + (lane4 + 256u * g)) : 0u;
    };
    auto unpack = [&](const uint32_t (&raw)[kRaw], float (&dst)[NE]) {
#pragma unroll
        for (int j = 0; j < NE; ++j)
            dst[j] = __uint_as_float(BF ? ((j & 1) ? raw[j >> 1] & 0xffff0000u : raw[j >> 1] << 16) : raw[BF ? 0 : j]);
    };
    // fixed-point scale of the privatised byte-table sums: chosen per workgroup from the upstream gradient rows of the
    // waves' first positions, v * 2^fx_k with the sample's max |g * scale_byte| at 2^27, so that a term converts through
    // a 32-bit integer.  Terms outside [2^12, 2^31) after scaling -- up to 16x the sample's maximum, down to 2^-15 of
    // it -- non-finite terms and rows without a slot take the exact global float atomic in a separate, rarely entered
    // block; the common path is straight-line (a term that must not be added there is replaced by zero).
    int fx_k = 0;
    uint32_t fx_lo_bits = 0, fx_span = 0;
    bool fx_known = !BYTES;
    auto byte_slot = [&](int id) { return id < A.priv_lo ? id : (id >= A.priv_hi0 ? id - A.priv_hi0 + A.priv_lo : -1); };
    auto in_range = [&](float v) { return ((__float_as_uint(v) & 0x7fffffffu) - fx_lo_bits) < fx_span; };
    // Within its LDS row, element wi sits at wi (fp32) or, for bf16, at wi / 2 + (wi odd ? Db / 2 : 0): a lane then holds the
    // elements 2 lane, 2 lane + 1, and with the even and the odd ones stored apart one ds_add_u64 touches consecutive
    // 8-byte words (stride-16 addresses would double the bank conflicts).  The flush at the end undoes the permutation.
    auto add_fixed = [&](int lrow, int j, float v) {   // lrow: byte offset of the row in dbyte_q (>= 0)
        const int q = __float2int_rn(ldexpf(v, fx_k));
        const int within = BF ? ((j & 1) ? wi4[j - 1] + (int)(row8 >> 1) : wi4[j]) : 2 * wi4[j];
        atomicAdd((unsigned long long *)((char *)dbyte_q + (uint32_t)(lrow + within)), (unsigned long long)(long long)q);
    };

    float acc[NE], an[NE];   // the current run: gradient of the token's table row so far, its (normalised) table row
    float ra = 1.f;          // 1 / rms of that row
    const float inv_dt = 1.0f / (float)A.Dt;
    int cur = -1;
    auto flush = [&]() {
        if (cur < 0 || (A.abl & 2)) return;
        char *drow = (char *)(A.d_tok + ((int64_t)cur * A.Dt - A.tok_lo));
#pragma unroll
        for (int j = 0; j < NE; ++j)
            if (tmask >> j & 1) atomicAdd((float *)(drow + (BF ? 2u * lane4 + 512u * (j >> 1) + 4u * (j & 1) : lane4 + 256u * j)), acc[j]);
    };
    auto load_id = [&](const int64_t *ids, int64_t n) {   // lanes < bpt: the token's byte ids, clamped once
        int64_t v = 0;
        if (lane < A.bpt) {
            v = *(const int64_t *)((const char *)(ids + n * A.bpt) + (uint32_t)lane * 8u);
            if ((uint64_t)v >= (uint64_t)A.byte_rows) { if (A.status) atomicOr(A.status, kStatusByteOor); v = 0; }
        }
        return (int)v;
    };
    // ---- positions come grouped by token id (A.pos_sorted / A.tok_sorted, the counting sort above): a workgroup takes a
    // contiguous share of the sorted order and a wave a contiguous eighth of that, so a token's positions form a run
    // inside a wave -- its table row is read once and its gradient row leaves with one atomic row-add per run (plus one
    // where a run crosses a wave boundary).  A wave reads 64 (position, token) pairs at a time and hands them out with
    // readlane, keeping the loop control scalar.
    const int64_t per_wg = (A.n_tokens + gridDim.x - 1) / gridDim.x;
    const int64_t wg_lo = min(A.n_tokens, (int64_t)blockIdx.x * per_wg), wg_hi = min(A.n_tokens, wg_lo + per_wg);
    const int64_t per_wave = (wg_hi - wg_lo + kBwdWaves - 1) / kBwdWaves;
    const int64_t s_begin = min(wg_hi, wg_lo + wave * per_wave), s_end = min(wg_hi, s_begin + per_wave);
    __syncthreads();   // orders the table zeroing above
    if (!fx_known) {   // uniform: every wave takes part, once per workgroup
        float gmax = 0.f;
        if (s_begin < s_end) {
            const char *grow = (const char *)A.grad_out + (int64_t)A.pos_sorted[s_begin] * D * (int64_t)esz;
            uint32_t gr[kRaw];
            float gs[NE];
            load_raw(grow, gr, 0xffffffffu);
            unpack(gr, gs);
#pragma unroll
            for (int j = 0; j < NE; ++j) gmax = fmaxf(gmax, fabsf(gs[j]));
            gmax = wave_max(gmax) * fabsf(s_byte);
            if (lane == 0 && gmax > 0.f && gmax < INFINITY) atomicMax(fx_bits, __float_as_uint(gmax));
        }
        __syncthreads();
        const float m = __uint_as_float(*fx_bits);
        fx_k = m > 0.f ? min(27 - ilogbf(m), 100) : 0;
        fx_lo_bits = __float_as_uint(ldexpf(1.0f, 12 - fx_k));
        fx_span = __float_as_uint(ldexpf(1.0f, 31 - fx_k)) - fx_lo_bits;
        fx_known = true;
    }
    for (int64_t s0 = s_begin; s0 < s_end; s0 += 64) {
        const int cnt = (int)min((int64_t)64, s_end - s0);
        int vpos = 0, vtok = 0;
        if (lane < cnt) { vpos = A.pos_sorted[s0 + lane]; vtok = A.tok_sorted[s0 + lane]; }
        int n_nx = __builtin_amdgcn_readfirstlane(vpos);
        int ida_nx = 0, idb_nx = 0;
        if (BYTES) {
            ida_nx = load_id(A.ids_a, n_nx);
            if (dual) idb_nx = load_id(A.ids_b, n_nx);
        }
        for (int k = 0; k < cnt; ++k) {
            const int64_t n = n_nx;
            const int tok = __builtin_amdgcn_readlane(vtok, k), ida = ida_nx, idb = idb_nx;
            const bool more = k + 1 < cnt;
            if (more) n_nx = __builtin_amdgcn_readlane(vpos, k + 1);

            float bn[NE], dy[NE];
            int lra[NE], lrb[NE];   // byte offset of the element's row in the LDS copy (negative: no slot), first / second id tensor
            const char *grow = (const char *)A.grad_out + n * D * (int64_t)esz;
            // The two element types get their own copy of the request / gather part: the bf16 one keeps raw dwords until
            // everything is in flight; folding both into one body cost the fp32 kernel 5 % (scheduling, not instruction count).
            if constexpr (BF) {
                uint32_t graw[kRaw], traw[kRaw], braw[kRaw], braw2[kRaw];
                load_raw(grow, graw, 0xffffffffu);
                if constexpr (!BF) unpack(graw, dy);
                const bool newrun = tok != cur;   // the previous token's gradient row leaves, this token's row comes in
                auto begin_run = [&]() {   // raw token row -> floats, its gradient accumulator, its rms factor
                    unpack(traw, an);
#pragma unroll
                    for (int j = 0; j < NE; ++j) acc[j] = 0.f;
                    ra = 1.f;
                    if (A.norm_tok) {
                        float ss = 0.f;
#pragma unroll
                        for (int j = 0; j < NE; ++j) ss += an[j] * an[j];
                        ra = rms_scale(wave_sum(ss), A.Dt, A.eps);
#pragma unroll
                        for (int j = 0; j < NE; ++j) an[j] *= ra;
                    }
                };
                if (newrun) {
                    flush();
                    cur = tok;
                    load_raw((const char *)A.tok_table + ((int64_t)tok * A.Dt - A.tok_lo) * (int64_t)esz, traw, tmask);
                    if constexpr (!BF) begin_run();   // fp32: nothing to unpack, the compiler places the waits at the first use
                }
                if (BYTES) {
                    // lanes < bpt: gather offset of the slot's byte row and offset of its LDS row (or -1)
                    const int ga = ida * A.Db * (int)esz, gb = idb * A.Db * (int)esz;
                    const int sa = byte_slot(ida), sb = byte_slot(idb);
                    const int la = sa >= 0 ? sa * (int)row8 : -1, lb = sb >= 0 ? sb * (int)row8 : -1;
#pragma unroll
                    for (int j = 0; j < NE; ++j) {
                        if (BF && (j & 1)) continue;   // a bf16 pair (j, j + 1) lies in one byte row: one permute, one dword gather
                        lra[j] = 0; lrb[j] = 0;
                        if constexpr (BF) {
                            const int g = j >> 1;
                            braw[g] = 0u; braw2[g] = 0u;
                            if (bmask >> j & 1) {
                                const uint32_t w = (uint32_t)wi4[j] >> 1;
                                braw[g] = *(const uint32_t *)((const char *)A.byte_table + ((uint32_t)__builtin_amdgcn_ds_bpermute(sl4[j], ga) + w));
                                lra[j] = __builtin_amdgcn_ds_bpermute(sl4[j], la);
                                if (dual) {
                                    braw2[g] = *(const uint32_t *)((const char *)A.byte_table + ((uint32_t)__builtin_amdgcn_ds_bpermute(sl4[j], gb) + w));
                                    lrb[j] = __builtin_amdgcn_ds_bpermute(sl4[j], lb);
                                }
                            }
                            if (j + 1 < NE) { lra[j + 1] = lra[j]; lrb[j + 1] = lrb[j]; }
                        } else {
                            bn[j] = 0.f;
                            if (!(bmask >> j & 1)) continue;
                            const uint32_t w = (uint32_t)wi4[j];
                            float v = *(const float *)((const char *)A.byte_table + ((uint32_t)__builtin_amdgcn_ds_bpermute(sl4[j], ga) + w));
                            lra[j] = __builtin_amdgcn_ds_bpermute(sl4[j], la);
                            if (dual) {
                                v += *(const float *)((const char *)A.byte_table + ((uint32_t)__builtin_amdgcn_ds_bpermute(sl4[j], gb) + w));
                                lrb[j] = __builtin_amdgcn_ds_bpermute(sl4[j], lb);
                            }
                            bn[j] = v;
                        }
                    }
                    if (more) {   // the next position's byte ids while this one's rows are in flight
                        ida_nx = load_id(A.ids_a, n_nx);
                        if (dual) idb_nx = load_id(A.ids_b, n_nx);
                    }
                }
                if constexpr (BF) {   // everything is requested: raw words -> floats
                    unpack(graw, dy);
                    if (BYTES) {
                        unpack(braw, bn);
                        if (dual) {
                            float b2[NE];
                            unpack(braw2, b2);
#pragma unroll
                            for (int j = 0; j < NE; ++j) bn[j] += b2[j];
                        }
                    }
                    if (newrun) begin_run();
                }
            } else {
#pragma unroll
                for (int j = 0; j < NE; ++j) dy[j] = *(const float *)(grow + (lane4 + 256u * j));
                if (tok != cur) {   // a new run: the previous token's gradient row leaves, this token's (normalised) row comes in
                    flush();
                    cur = tok;
                    const char *trow = (const char *)A.tok_table + ((int64_t)tok * A.Dt - A.tok_lo) * (int64_t)esz;
#pragma unroll
                    for (int j = 0; j < NE; ++j) {
                        acc[j] = 0.f;
                        an[j] = (tmask >> j & 1) ? *(const float *)(trow + (lane4 + 256u * j)) : 0.f;
                    }
                    ra = 1.f;
                    if (A.norm_tok) {
                        float ss = 0.f;
#pragma unroll
                        for (int j = 0; j < NE; ++j) ss += an[j] * an[j];
                        ra = rms_scale(wave_sum(ss), A.Dt, A.eps);
#pragma unroll
                        for (int j = 0; j < NE; ++j) an[j] *= ra;
                    }
                }
                if (BYTES) {
                    // lanes < bpt: gather offset of the slot's byte row and offset of its LDS row (or -1)
                    const int ga = ida * A.Db * (int)esz, gb = idb * A.Db * (int)esz;
                    const int sa = byte_slot(ida), sb = byte_slot(idb);
                    const int la = sa >= 0 ? sa * (int)row8 : -1, lb = sb >= 0 ? sb * (int)row8 : -1;
#pragma unroll
                    for (int j = 0; j < NE; ++j) {
                        bn[j] = 0.f; lra[j] = 0; lrb[j] = 0;
                        if (!(bmask >> j & 1)) continue;
                        const uint32_t w = (uint32_t)wi4[j];
                        float v = *(const float *)((const char *)A.byte_table + ((uint32_t)__builtin_amdgcn_ds_bpermute(sl4[j], ga) + w));
                        lra[j] = __builtin_amdgcn_ds_bpermute(sl4[j], la);
                        if (dual) {
                            v += *(const float *)((const char *)A.byte_table + ((uint32_t)__builtin_amdgcn_ds_bpermute(sl4[j], gb) + w));
                            lrb[j] = __builtin_amdgcn_ds_bpermute(sl4[j], lb);
                        }
                        bn[j] = v;
                    }
                    if (more) {   // the next position's byte ids while this one's rows are in flight
                        ida_nx = load_id(A.ids_a, n_nx);
                        if (dual) idb_nx = load_id(A.ids_b, n_nx);
                    }
                }
            }
            float rnb = 1.f;   // lanes < bpt: 1/rms of the slot's byte row
            if (BYTES && A.norm_byte) {
                if (pair_norm) {   // the rms factor belongs to the (token, slot) pair: per-slot sum of squares in fixed point
                    float pmax = 0.f;
#pragma unroll
                    for (int j = 0; j < NE; ++j) pmax = fmaxf(pmax, bn[j] * bn[j]);
                    pmax = wave_max(pmax);
                    const int kk = (pmax > 0.f && pmax < INFINITY) ? 40 - ilogbf(pmax) : 0;
                    seg_q[lane] = 0ull;
                    seg_sync();
#pragma unroll
                    for (int j = 0; j < NE; ++j)
                        if (bmask >> j & 1) atomicAdd(seg_q + (sl4[j] >> 2), to_fixed(bn[j] * bn[j], kk));
                    seg_sync();
                    rnb = rms_scale((float)ldexp((double)(long long)seg_q[lane], -kk), A.Db, A.eps);
                    seg_sync();
                } else {
                    rnb = A.byte_rnorm[ida];
                }
#pragma unroll
                for (int j = 0; j < NE; ++j) bn[j] *= __int_as_float(__builtin_amdgcn_ds_bpermute(sl4[j], __float_as_int(rnb)));
            }
            // ---- back through the output norm
            if (A.norm_out) {
                float ss = 0.f, m = 0.f;
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const float y = an[j] * s_tok + (mixes_bytes(MODE) ? bn[j] * s_byte : 0.f);
                    ss += y * y;
                    m += dy[j] * y;
                }
                const float ry = rms_scale(wave_sum(ss), D, A.eps);
                m = wave_sum(m) * ry * (1.0f / (float)D);       // mean(g * x), x = y * ry   (a multiply, not an IEEE divide: <= 1 ulp)
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const float x = (an[j] * s_tok + (mixes_bytes(MODE) ? bn[j] * s_byte : 0.f)) * ry;
                    dy[j] = ry * (dy[j] - x * m);
                }
            }
            // ---- token side
            {
                float dot = 0.f;
#pragma unroll
                for (int j = 0; j < NE; ++j) dot += dy[j] * an[j];
                ds_t += dot;
                float mt = 0.f;
                if (A.norm_tok) mt = wave_sum(dot * s_tok) * inv_dt;
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    const float da = dy[j] * s_tok;
                    acc[j] += A.norm_tok ? ra * (da - an[j] * mt) : da;
                }
            }
            // ---- byte side
            if (BYTES) {
                float dot = 0.f;
#pragma unroll
                for (int j = 0; j < NE; ++j) { dot += dy[j] * bn[j]; dy[j] *= s_byte; }
                ds_b += dot;
                if (A.norm_byte) {   // v = r_row * (db - b_n * mean_slot(db * b_n)): per-slot sums in fixed point
                    float pmax = 0.f;
#pragma unroll
                    for (int j = 0; j < NE; ++j) pmax = fmaxf(pmax, fabsf(dy[j] * bn[j]));
                    pmax = wave_max(pmax);
                    const int kk = (pmax > 0.f && pmax < INFINITY) ? 40 - ilogbf(pmax) : 0;
                    // every lane takes part in the zeroing and the read-back (kMaxBpt = 64 entries): with a
                    // `lane < bpt` guard the compiler sinks the atomics into both sides of the branch and the
                    // unguarded lanes' adds run BEFORE the zeroing store
                    seg_q[lane] = 0ull;
                    seg_sync();
#pragma unroll
                    for (int j = 0; j < NE; ++j)
                        if (bmask >> j & 1) atomicAdd(seg_q + (sl4[j] >> 2), to_fixed(dy[j] * bn[j], kk));
                    seg_sync();
                    float sg = (float)ldexp((double)(long long)seg_q[lane], -kk) / (float)A.Db;
                    if (!(pmax < INFINITY)) sg = NAN;   // non-finite gradients stay non-finite
#pragma unroll
                    for (int j = 0; j < NE; ++j) {
                        const float rj = __int_as_float(__builtin_amdgcn_ds_bpermute(sl4[j], __float_as_int(rnb)));
                        const float sj = __int_as_float(__builtin_amdgcn_ds_bpermute(sl4[j], __float_as_int(sg)));
                        dy[j] = rj * (dy[j] - bn[j] * sj);
                    }
                    seg_sync();
                }
                if (!(A.abl & 1)) {
                    bool slow = false;   // some element of this lane needs the exact path
#pragma unroll
                    for (int j = 0; j < NE; ++j) {
                        if (!(bmask >> j & 1)) continue;
                        const bool inr = in_range(dy[j]), nz = (__float_as_uint(dy[j]) << 1) != 0u;
                        const bool oka = inr && lra[j] >= 0;
                        add_fixed(max(lra[j], 0), j, oka ? dy[j] : 0.f);
                        slow |= nz && !oka;
                        if (dual) {
                            const bool okb = inr && lrb[j] >= 0;
                            add_fixed(max(lrb[j], 0), j, okb ? dy[j] : 0.f);
                            slow |= nz && !okb;
                        }
                    }
                    if (__any(slow)) {
#pragma unroll
                        for (int j = 0; j < NE; ++j) {
                            if (!(bmask >> j & 1)) continue;
                            const bool inr = in_range(dy[j]), nz = (__float_as_uint(dy[j]) << 1) != 0u;
                            const int wi = wi4[j] >> 2;
                            const int ia = __builtin_amdgcn_ds_bpermute(sl4[j], ida);
                            if (nz && !(inr && lra[j] >= 0)) atomicAdd(A.d_byte + ia * A.Db + wi, dy[j]);
                            if (dual) {
                                const int ib = __builtin_amdgcn_ds_bpermute(sl4[j], idb);
                                if (nz && !(inr && lrb[j] >= 0)) atomicAdd(A.d_byte + ib * A.Db + wi, dy[j]);
                            }
                        }
                    }
                }
            }
        }
    }
    flush();
    if (A.d_scale_tok) { ds_t = wave_sum(ds_t); if (lane == 0) atomicAdd(A.d_scale_tok, ds_t); }
    if (BYTES && A.d_scale_byte) { ds_b = wave_sum(ds_b); if (lane == 0) atomicAdd(A.d_scale_byte, ds_b); }
    if (BYTES) {
        __syncthreads();
        for (int i = tid; i < nbyte; i += kBwdThreads) {
            const long long q = (long long)dbyte_q[i];
            if (q == 0) continue;
            const int sl = i / A.Db, at = i - sl * A.Db, half = A.Db >> 1;
            const int wi = BF ? (at < half ? 2 * at : 2 * (at - half) + 1) : at;
            const int row = sl < A.priv_lo ? sl : sl - A.priv_lo + A.priv_hi0;
            atomicAdd(A.d_byte + row * A.Db + wi, (float)ldexp((double)q, -fx_k));
        }
    }
}

// ------------------------------------------------------------------------------------------
// Lane-contiguous variant for the headline shapes: SUM / NOOP, fp32, D = 64 NE with NE a multiple of 4, and (SUM) a byte slot
// made of whole lanes (Db a multiple of NE, i.e. 64 / bpt lanes per slot: bpt a power of two).  A lane owns NE CONSECUTIVE
// elements of a row, so
//   * a gradient row, a token row and the lane's piece of a byte row are NE / 4 16-byte loads each (the strided layout of
//     embed_mix_bwd_full_kernel needs NE 4-byte loads: four times the vector-memory instructions per position, and the
//     position rate of that kernel was what its address unit could issue);
//   * a lane belongs to ONE byte slot: one id, one row offset, one rms factor per lane, no cross-lane hand-out; the per-slot
//     sums of the byte-norm backward are a lane-local sum plus a log2(64 / bpt)-step exchange inside the slot's lane group;
//   * 12 waves per workgroup (one workgroup per CU: the privatised byte-table gradient takes most of the LDS), each with the
//     NEXT position's gradient row already requested while it works on the current one: the kernel streams 1.6 GB of gradient
//     rows, and one 3 KB row in flight per wave (16 waves: 48 KB per CU) covered 60 % of what HBM latency x bandwidth asks for;
//   * the privatised table's rows are Db + 1 sums apart: with a stride of Db = 48 64-bit words every row starts on one of two
//     bank offsets and a wave's 64 adds met on 8 bank positions (SQ_LDS_BANK_CONFLICT was a quarter of the kernel's cycles).
// The token-table flush wants 256 contiguous bytes per atomic wave-instruction (lane-contiguous pieces would spread each
// instruction over 3 KB: ~12x the memory-side atomic requests), so a run's gradient row is transposed through a per-wave LDS
// buffer once per run (a run of equal tokens is ~17 positions long on FineWeb-shaped ids).
// ------------------------------------------------------------------------------------------
constexpr int kLcThreads = 768, kLcWaves = kLcThreads / 64;   // 12 waves, 3 per SIMD: ~170 registers per lane, room for the next position's gradient row

// T: the element type of the tables and of grad_out (float, or __bf16: rows widened as they are loaded; every sum stays fp32)
template <int MODE, int NE, bool DUAL, typename T>
__global__ __launch_bounds__(kLcThreads) void embed_mix_bwd_lc_kernel(const BwdArgs A) {
#pragma clang fp contract(fast)   // fused multiply-adds here: the sums below are compared with float64 at 2e-5, not bit for bit
    constexpr int D = 64 * NE, NV = NE / 4;
    constexpr bool BYTES = MODE != MOT_MIX_NOOP;
    extern __shared__ unsigned long long lds_q[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qs = A.Db + 1;                                      // row stride of the privatised sums, in 64-bit words
    const int nbyte = (A.priv_rows * qs + 1) & ~1;
    unsigned long long *dbyte_q = lds_q;
    uint32_t *fx_bits = (uint32_t *)(lds_q + nbyte);
    float *xp = (float *)(lds_q + nbyte + 2) + wave * D;          // this wave's transposition buffer (16-byte aligned: nbyte is even)
    for (int i = tid; i < nbyte; i += kLcThreads) dbyte_q[i] = 0ull;
    if (tid == 0) *fx_bits = 0u;
    const float s_tok = A.scale_tok ? *A.scale_tok : 1.0f;
    const float s_byte = A.scale_byte ? *A.scale_byte : 1.0f;
    const float inv_d = 1.0f / (float)D;
    // the lane's place: byte slot, first element inside the slot's row
    const int lps = BYTES ? A.Db / NE : 64;                       // lanes per slot
    const int slot = BYTES ? lane / lps : 0;
    const int wi0 = BYTES ? (lane - slot * lps) * NE : 0;
    const uint32_t lane_off = (uint32_t)lane * (NE * (uint32_t)sizeof(T));
    const T *grad_out = (const T *)A.grad_out, *tok_table = (const T *)A.tok_table, *byte_table = (const T *)A.byte_table;
    const int64_t gld = A.g_ld ? A.g_ld : D;                      // elements between gradient rows
    const bool no_tok = A.no_tok != 0;                            // byte slots only: no token row is read, none is written
    auto load_row = [&](const char *rbase, float (&dst)[NE]) {   // NE consecutive elements at rbase + lane_off
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float4v w = Elem<T>::load4((const T *)(rbase + (lane_off + 4u * (uint32_t)sizeof(T) * v)));
            dst[4 * v] = w.x; dst[4 * v + 1] = w.y; dst[4 * v + 2] = w.z; dst[4 * v + 3] = w.w;
        }
    };
    auto load_byte_row = [&](int id, float (&dst)[NE]) { load_row((const char *)(byte_table + (int64_t)id * A.Db + wi0) - lane_off, dst); };
    auto slot_sum = [&](float v) {                                // sum over the lanes of this lane's slot (lps a power of two)
        for (int o = 1; o < lps; o <<= 1) v += __shfl_xor(v, o, 64);
        return v;
    };
    int fx_k = 0;
    bool fx_on = false;                                           // a non-zero finite sample exists: without one NOTHING is converted
    float fx_mul = 1.f;                                           // s_byte * 2^fx_k: a byte-row term's fixed-point value is dy * fx_mul
    auto byte_slot = [&](int id) { return id < A.priv_lo ? id : (id >= A.priv_hi0 ? id - A.priv_hi0 + A.priv_lo : -1); };

    float acc[NE], an[NE];
    float ra = 1.f, ds_t = 0.f, ds_b = 0.f;
    int cur = -1;
    auto flush = [&]() {
        if (cur < 0 || no_tok) return;
#pragma unroll
        for (int v = 0; v < NV; ++v) *(float4v *)(xp + lane * NE + 4 * v) = float4v{acc[4 * v], acc[4 * v + 1], acc[4 * v + 2], acc[4 * v + 3]};
        seg_sync();
        float *drow = A.d_tok + (int64_t)cur * D;
#pragma unroll
        for (int j = 0; j < NE; ++j) atomicAdd(drow + lane + 64 * j, xp[lane + 64 * j]);
        seg_sync();
    };
    const int64_t per_wg = (A.n_tokens + gridDim.x - 1) / gridDim.x;
    const int64_t wg_lo = min(A.n_tokens, (int64_t)blockIdx.x * per_wg), wg_hi = min(A.n_tokens, wg_lo + per_wg);
    const int64_t per_wave = (wg_hi - wg_lo + kLcWaves - 1) / kLcWaves;
    const int64_t s_begin = min(wg_hi, wg_lo + wave * per_wave), s_end = min(wg_hi, s_begin + per_wave);
    __syncthreads();   // orders the table zeroing above
    if (BYTES) {       // fixed-point scale of the privatised sums, as in embed_mix_bwd_full_kernel: every wave takes part
        float gmax = 0.f;
        if (s_begin < s_end) {
            float gs[NE];
            load_row((const char *)(grad_out + (int64_t)A.pos_sorted[s_begin] * gld), gs);
#pragma unroll
            for (int j = 0; j < NE; ++j) gmax = fmaxf(gmax, fabsf(gs[j]));
            gmax = wave_max(gmax) * fabsf(s_byte);
            if (lane == 0 && gmax > 0.f && gmax < INFINITY) atomicMax(fx_bits, __float_as_uint(gmax));
        }
        __syncthreads();
        const float m = __uint_as_float(*fx_bits);
        fx_on = m > 0.f;
        fx_k = fx_on ? max(-100, min(27 - ilogbf(m), 100)) : 0;
        fx_mul = ldexpf(s_byte, fx_k);
    }
    // the id of this lane's slot: requested raw, range-checked where it is first used (a check right behind the load would make
    // the wave wait for everything it has in flight)
    auto load_id = [&](const int64_t *ids, int64_t n) { return *(const int64_t *)((const char *)(ids + n * A.bpt + A.slot0) + (uint32_t)slot * 8u); };
    auto clamp_id = [&](int64_t v) {
        if ((uint64_t)v >= (uint64_t)A.byte_rows) { if (A.status) atomicOr(A.status, kStatusByteOor); v = 0; }
        return (int)v;
    };
    // Three positions are in flight per wave: k is being worked on, the rows of k + 1 (gradient row, byte rows) and the byte
    // ids of k + 2 have been requested.  Positions come 64 (position, token) pairs at a time, handed out with readlane.
    for (int64_t s0 = s_begin; s0 < s_end; s0 += 64) {
        const int cnt = (int)min((int64_t)64, s_end - s0);
        int vpos = 0, vtok = 0;
        if (lane < cnt) { vpos = A.pos_sorted[s0 + lane]; vtok = A.tok_sorted[s0 + lane]; }
        const int n0 = __builtin_amdgcn_readfirstlane(vpos), n1 = __builtin_amdgcn_readlane(vpos, cnt > 1 ? 1 : 0);
        float g_nx[NE], b_nx[NE], rn_nx = 1.f;
        int ida_nx = 0, idb_nx = 0;
        int64_t ida_n2 = 0, idb_n1 = 0;                           // raw: the first id tensor's entry two positions ahead, the second's one ahead
        load_row((const char *)(grad_out + (int64_t)n0 * gld), g_nx);
        if (BYTES) {
            ida_nx = clamp_id(load_id(A.ids_a, n0));
            if (DUAL) idb_nx = clamp_id(load_id(A.ids_b, n0));
            ida_n2 = load_id(A.ids_a, n1);
            if (DUAL) idb_n1 = load_id(A.ids_b, n1);
            load_byte_row(ida_nx, b_nx);
            if (A.norm_byte) rn_nx = A.byte_rnorm[ida_nx];
        }
        for (int k = 0; k < cnt; ++k) {
            const int tok = __builtin_amdgcn_readlane(vtok, k), ida = ida_nx, idb = idb_nx;
            const bool more = k + 1 < cnt, newrun = tok != cur;
            float dy[NE], bn[NE];
            const float rnb = rn_nx;
#pragma unroll
            for (int j = 0; j < NE; ++j) { dy[j] = g_nx[j]; bn[j] = BYTES ? b_nx[j] : 0.f; }
            // Requests are issued oldest-needed first (a wave's loads return in order): what THIS position still lacks -- a new
            // run's token row, the second id tensor's byte row -- goes out before the next position's rows, so that waiting for
            // it leaves those in flight.
            float b2[NE];
            if constexpr (DUAL) load_byte_row(idb, b2);
            if (newrun) {   // the previous token's gradient row leaves, this token's row comes in
                flush();
                cur = tok;
                if (no_tok) {
#pragma unroll
                    for (int j = 0; j < NE; ++j) an[j] = 0.f;
                } else load_row((const char *)(tok_table + (int64_t)tok * D), an);
            }
            if (more) {   // the next position's rows, the byte ids of the one after
                const int nn = __builtin_amdgcn_readlane(vpos, k + 1);
                load_row((const char *)(grad_out + (int64_t)nn * gld), g_nx);
                if (BYTES) {
                    ida_nx = clamp_id(ida_n2);
                    if (DUAL) idb_nx = clamp_id(idb_n1);
                    load_byte_row(ida_nx, b_nx);
                    if (A.norm_byte) rn_nx = A.byte_rnorm[ida_nx];
                    if (k + 2 < cnt) {
                        const int n2 = __builtin_amdgcn_readlane(vpos, k + 2);
                        ida_n2 = load_id(A.ids_a, n2);
                        if (DUAL) idb_n1 = load_id(A.ids_b, n2);
                    }
                }
            }
            if constexpr (DUAL) {
#pragma unroll
                for (int j = 0; j < NE; ++j) bn[j] += b2[j];
            }
            if (newrun) {
#pragma unroll
                for (int j = 0; j < NE; ++j) acc[j] = 0.f;
                ra = 1.f;
                if (A.norm_tok) {
                    float ss = 0.f;
#pragma unroll
                    for (int j = 0; j < NE; ++j) ss += an[j] * an[j];
                    ra = rms_scale(wave_sum(ss), D, A.eps);
#pragma unroll
                    for (int j = 0; j < NE; ++j) an[j] *= ra;
                }
            }
            if (BYTES && A.norm_byte) {
#pragma unroll
                for (int j = 0; j < NE; ++j) bn[j] *= rnb;
            }
            // ---- back through the output norm: x = ry y, dy = ry (g - x mean(g x)) = ry g - (ry^3 sum(g y) / D) y
            if (A.norm_out) {
                float y[NE], ss = 0.f, m = 0.f;
#pragma unroll
                for (int j = 0; j < NE; ++j) {
                    y[j] = BYTES ? an[j] * s_tok + bn[j] * s_byte : an[j] * s_tok;
                    ss += y[j] * y[j];
                    m += dy[j] * y[j];
                }
                const float ry = rms_scale(wave_sum(ss), D, A.eps);
                const float c2 = wave_sum(m) * inv_d * ry * ry * ry;
#pragma unroll
                for (int j = 0; j < NE; ++j) dy[j] = ry * dy[j] - c2 * y[j];
            }
            // ---- token side
            {
                float dot = 0.f;
#pragma unroll
                for (int j = 0; j < NE; ++j) dot += dy[j] * an[j];
                ds_t += dot;
                if (A.norm_tok) {
                    const float c = wave_sum(dot) * s_tok * inv_d, rs = ra * s_tok;   // ra (s_t dy - a_n mean(s_t dy . a_n))
#pragma unroll
                    for (int j = 0; j < NE; ++j) acc[j] += rs * dy[j] - (ra * c) * an[j];
                } else {
#pragma unroll
                    for (int j = 0; j < NE; ++j) acc[j] += dy[j] * s_tok;
                }
            }
            // ---- byte side
            if (BYTES) {
                float dot = 0.f;
#pragma unroll
                for (int j = 0; j < NE; ++j) dot += dy[j] * bn[j];
                ds_b += dot;
                if (A.norm_byte) {   // v = r_row (db - b_n mean_slot(db b_n)), db = s_b dy: the slot is this lane's group
                    const float sg = slot_sum(dot) / (float)A.Db;
#pragma unroll
                    for (int j = 0; j < NE; ++j) dy[j] = rnb * (dy[j] - bn[j] * sg);
                }
                // Fixed-point sums in LDS: x = dy s_b 2^fx_k rounded to a 32-bit integer, added into 64-bit words.  A lane takes
                // this path with all its NE terms or not at all: it must have an LDS row, the workgroup must have a scale (a
                // non-zero finite sample: with all sampled rows zero, 2^0 would round every |term| < 0.5 away), and its largest |x|
                // must lie in [2^12, 2^31) -- or be zero, which adds nothing.  The upper bound is what converts (the comparison is
                // made on the |x| BIT PATTERNS, which order NaN above infinity: v_max_f32 would drop a NaN); the lower bound keeps
                // rows far below the sample (masked or down-weighted positions: largest term <= 2^-15 of the sampled maximum) on
                // the float atomics with their full relative precision.  Inside a converted lane a term's absolute rounding error
                // is <= 2^-(fx_k + 1), i.e. 2^-28 of the sampled |g s_b| maximum -- below what a float atomic loses on a row's
                // running sum.  Lanes that fail add exact global float atomics instead.
                const int sa = byte_slot(ida), sb = DUAL ? byte_slot(idb) : 0;
                uint32_t abits = 0u;
#pragma unroll
                for (int j = 0; j < NE; ++j) { dy[j] *= fx_mul; abits = max(abits, __float_as_uint(dy[j]) & 0x7fffffffu); }
                const bool fits = fx_on && abits < 0x4f000000u /* 2^31 */ && abits >= 0x45800000u /* 2^12 */, zero = abits == 0u;
                const bool oka = zero || (fits && sa >= 0), okb = DUAL ? (zero || (fits && sb >= 0)) : true;
                if (__all(oka && okb)) {   // (an all-zero lane may have no LDS row: it adds zeros to row 0)
                    unsigned long long *ra_q = dbyte_q + (size_t)max(sa, 0) * qs + wi0, *rb_q = dbyte_q + (size_t)max(sb, 0) * qs + wi0;
#pragma unroll
                    for (int j = 0; j < NE; ++j) {
                        const unsigned long long q = (unsigned long long)(long long)__float2int_rn(dy[j]);
                        atomicAdd(ra_q + j, q);
                        if (DUAL) atomicAdd(rb_q + j, q);
                    }
                } else {
                    const float back = ldexpf(1.0f, -fx_k);       // x 2^-fx_k: the term itself, exactly
                    unsigned long long *ra_q = dbyte_q + (size_t)max(sa, 0) * qs + wi0, *rb_q = dbyte_q + (size_t)max(sb, 0) * qs + wi0;
#pragma unroll
                    for (int j = 0; j < NE; ++j) {
                        const unsigned long long q = (unsigned long long)(long long)__float2int_rn(fits ? dy[j] : 0.f);
                        const float v = dy[j] * back;
                        if (oka) atomicAdd(ra_q + j, q); else if (v != 0.f) atomicAdd(A.d_byte + (int64_t)ida * A.Db + wi0 + j, v);
                        if (DUAL) { if (okb) atomicAdd(rb_q + j, q); else if (v != 0.f) atomicAdd(A.d_byte + (int64_t)idb * A.Db + wi0 + j, v); }
                    }
                }
            }
        }
    }
    flush();
    if (A.d_scale_tok) { ds_t = wave_sum(ds_t); if (lane == 0) atomicAdd(A.d_scale_tok, ds_t); }
    if (BYTES && A.d_scale_byte) { ds_b = wave_sum(ds_b); if (lane == 0) atomicAdd(A.d_scale_byte, ds_b); }
    if (BYTES) {
        __syncthreads();
        for (int i = tid; i < A.priv_rows * A.Db; i += kLcThreads) {
            const int sl = i / A.Db, wi = i - sl * A.Db;
            const long long q = (long long)dbyte_q[sl * qs + wi];
            if (q == 0) continue;
            const int row = sl < A.priv_lo ? sl : sl - A.priv_lo + A.priv_hi0;
            atomicAdd(A.d_byte + row * A.Db + wi, (float)ldexp((double)q, -fx_k));
        }
    }
}

template <int MODE>
static bool lc_layout(const BwdArgs &A) {
    if ((A.D & 255) || A.Dt != A.D || A.tok_lo != 0 || A.D > 1024) return false;
    const int ne = A.D / 64;
    if (MODE == MOT_MIX_SUM) {
        if (A.byte_lo != 0 || A.nbk != A.D || A.Db % ne) return false;
        const int lps = A.Db / ne;
        if (lps & (lps - 1)) return false;                        // the slot sums exchange inside power-of-two lane groups
        if (A.ids_b && ne > 12) return false;                     // two id tensors at 1024 columns would spill
    }
    return ne == 4 || ne == 8 || ne == 12 || ne == 16;   // 1024-thread workgroups cap a lane at 128 registers: NE 24 / 32 would spill
}

template <int MODE, int NE, bool DUAL>
static int launch_bwd_lc_t(const BwdArgs &A, size_t lds, hipStream_t stream) {
    const int64_t blocks = (A.n_tokens + 16 * kLcWaves - 1) / (16 * kLcWaves);   // >= 16 sorted positions per wave
    if (A.in_bf16) return launch_scatter<embed_mix_bwd_lc_kernel<MODE, NE, DUAL, __bf16>>(A, lds, stream, kLcThreads, blocks, "embed_mix_bwd_lc_kernel");
    return launch_scatter<embed_mix_bwd_lc_kernel<MODE, NE, DUAL, float>>(A, lds, stream, kLcThreads, blocks, "embed_mix_bwd_lc_kernel");
}
template <int MODE, int NE>
static int launch_bwd_lc(const BwdArgs &A, size_t lds, hipStream_t stream) {
    if constexpr (MODE == MOT_MIX_SUM) {
        if (A.ids_b) return launch_bwd_lc_t<MODE, NE, true>(A, lds, stream);
    }
    return launch_bwd_lc_t<MODE, NE, false>(A, lds, stream);
}

template <int MODE>
static int dispatch_ne_lc(const BwdArgs &A, size_t lds, hipStream_t stream) {
    switch (A.D / 64) {
        case 4: return launch_bwd_lc<MODE, 4>(A, lds, stream);
        case 8: return launch_bwd_lc<MODE, 8>(A, lds, stream);
        case 12: return launch_bwd_lc<MODE, 12>(A, lds, stream);
        default: return launch_bwd_lc<MODE, 16>(A, lds, stream);
    }
}

// ------------------------------------------------------------------------------------------
// Round 3: the headline configuration by itself.  norm(E_tok[t] + concat_k E_byte[id_k]) of runs/71_*.py:227-230 has no
// per-embedding norm and no learned scalar, so nothing of the general kernel's token / byte side bookkeeping is needed:
//     y = a + b,   dy = ry g - (ry^3 mean(g y)) y,   d_tok[t] += dy,   d_byte[id_k] += dy[slot k]
// What the counters and timing ablations said about embed_mix_bwd_lc_kernel on this configuration (profiles/r03_c4_backward_*):
// its HBM traffic IS the algorithmic traffic (FETCH 1.81 GB + WRITE 0.18 GB + 0.19 GB of atomic requests against 1.61 GB of
// gradient rows + token rows + ids); the LDS adds cost 0.03-0.05 ms, the token-row flushes 0.10 ms, everything else 0.34 ms
// (1.8 GB of random 3 KB rows at 5.4 TB/s, the rate the CDNA guide measures for such gathers), and the parts do not overlap.
// This kernel changes what could be changed inside hipcc's own s_waitcnt placement:
//   * rows are read as 16-byte chunks lane, lane + 64, ...: every row load is a fully coalesced 1 KiB wave-instruction that
//     touches each 128-byte line once (the lane-contiguous layout reads a row with NV instructions that each touch all of its
//     lines; with more rows in flight than the 32 KB L1 holds, lines are fetched up to three times -- requesting rows further
//     ahead made that kernel SLOWER);
//   * the current run's token row lives in the wave's LDS strip (NV ds_read_b128 per place instead of NE registers), the bpt
//     ids of a place are ONE 8-byte load per lane handed out with ds_bpermute, the running sum and the byte-row terms share one
//     scaled form (dys = 2^k dy feeds both the fixed-point LDS adds and the register sum);
//   * lookahead indices are clamped inside a 128-place segment, so every step issues the same requests, and the step is
//     written twice (same run / new run): hipcc counts its waits per straight-line path and takes the SMALLER count wherever
//     two paths join, so one shared body made every step wait for the gradient row of the NEXT place.
// What is left on the table, measured ("Backward, round 3"): a new run still drains the wave's memory queue
// (the compiler-visible token-row load behind the 12 atomics: two memory round trips per run, 17 runs per wave, 0.10 ms); the
// versions that avoid it -- atomics or a plain read-add-store of the d_tok row at the END of the step, requests from inline asm
// with hand-counted vmcnt -- lost to hipcc copying in-flight registers in front of the tied waits (v_mov_b64 of the id pair, then
// the wait on the copy; with physical-register constraints: copies in and out of the pinned registers and 46 spills).
// Everything else -- the sorted order, the privatised 64-bit byte-table sums with 49-word rows, the exact global-atomic path
// for what has no LDS slot or does not convert -- is embed_mix_bwd_lc_kernel's.
// ------------------------------------------------------------------------------------------
constexpr int kPlThreads = 768, kPlWaves = kPlThreads / 64;   // 12 waves, 3 per SIMD: 168 registers per lane

// T: element type of the tables and of grad_out (float, or __bf16 as the production loop runs them, train_gpt.py:1124-1126); all
// arithmetic and every gradient buffer are fp32.  A lane's chunk is FOUR elements either way (16 bytes of fp32, 8 bytes of bf16).
template <int MODE, int NE, bool NORM_OUT, typename T>
__global__ __launch_bounds__(kPlThreads) void embed_mix_bwd_plain_kernel(const BwdArgs A) {
#pragma clang fp contract(fast)
    constexpr int D = 64 * NE, NV = NE / 4;
    constexpr bool BYTES = MODE != MOT_MIX_NOOP;
    constexpr int kSeg = 128;                                     // places per pipeline segment: their (position, token) pairs sit in 2 x 2 registers
#ifdef MOT_DEV_ABLATION   // timing-only switches (results are wrong): 1 no LDS byte adds, 2 no token-row atomics, 512 no wave sums
#define PL_ABL(bit) (A.abl & (bit))
#else
#define PL_ABL(bit) false
#endif
    extern __shared__ unsigned long long lds_q[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qs = A.Db + 1;
    const int nbyte = (A.priv_rows * qs + 1) & ~1;
    unsigned long long *dbyte_q = lds_q;
    uint32_t *fx_bits = (uint32_t *)(lds_q + nbyte);
    float *xp = (float *)(lds_q + nbyte + 2) + wave * D;
    for (int i = tid; i < nbyte; i += kPlThreads) dbyte_q[i] = 0ull;
    if (tid == 0) *fx_bits = 0u;
    const float inv_d = 1.0f / (float)D;
    // Lane l owns the 16-byte chunks l, l + 64, ... of a row (elements 4c .. 4c + 3 of chunk c).  A chunk lies inside one byte
    // slot (Db a multiple of 4): chunk v of this lane belongs to slot sl[v] and starts at element wo[v] of that slot's byte row.
    const int cps = BYTES ? A.Db / 4 : 1;                         // chunks per slot
    int sl[NV], wo[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) { const int c = lane + 64 * v; sl[v] = BYTES ? c / cps : 0; wo[v] = BYTES ? 4 * (c - sl[v] * cps) : 0; }
    constexpr uint32_t kChunk = 4u * (uint32_t)sizeof(T);          // bytes of a lane's chunk in the tables / grad_out
    const uint32_t lane_off = (uint32_t)lane * kChunk;
    const T *tok_table = (const T *)A.tok_table, *byte_table = (const T *)A.byte_table, *grad_out = (const T *)A.grad_out;
    auto load_row = [&](float4v (&dst)[NV], const T *rbase) {     // one row of D elements in chunk order, widened
#pragma unroll
        for (int v = 0; v < NV; ++v) dst[v] = Elem<T>::load4((const T *)((const char *)rbase + (lane_off + 64u * kChunk * v)));
    };
    auto load_byte_rows = [&](float4v (&dst)[NV], const int (&id)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; ++v) dst[v] = Elem<T>::load4(byte_table + (int64_t)id[v] * A.Db + wo[v]);
    };
    auto byte_slot = [&](int id) { return id < A.priv_lo ? id : (id >= A.priv_hi0 ? id - A.priv_hi0 + A.priv_lo : -1); };
    // The bpt ids of a position are one cache line: lane k < bpt loads id k (one 8-byte load per position), range-checks it, and
    // the NV slots of every lane pick theirs with ds_bpermute (the LDS crossbar: no memory, no bank conflicts).
    const int idl = min(lane, max(A.bpt, 1) - 1);
    auto load_ids = [&](int64_t n) { return A.ids_a[n * A.bpt + idl]; };
    auto clamp_id = [&](int64_t raw) {
        const bool bad = (uint64_t)raw >= (uint64_t)A.byte_rows;
        if (bad && A.status) atomicOr(A.status, kStatusByteOor);
        return bad ? 0 : (int)raw;
    };
    auto spread_ids = [&](int idv, int (&id)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; ++v) id[v] = __builtin_amdgcn_ds_bpermute(sl[v] * 4, idv);
    };
    const int64_t per_wg = (A.n_tokens + gridDim.x - 1) / gridDim.x;
    const int64_t wg_lo = min(A.n_tokens, (int64_t)blockIdx.x * per_wg), wg_hi = min(A.n_tokens, wg_lo + per_wg);
    const int64_t per_wave = (wg_hi - wg_lo + kPlWaves - 1) / kPlWaves;
    const int64_t s_begin = min(wg_hi, wg_lo + wave * per_wave), s_end = min(wg_hi, s_begin + per_wave);
    __syncthreads();
    // fixed-point scale 2^fx_k of the privatised sums from one sampled gradient row per wave (sample maximum -> 2^27); with no
    // non-zero finite sample (m == 0) NOTHING takes the fixed-point path: every non-zero term goes out as an exact float atomic
    int fx_k = 0;
    bool fx_on = false;
    {
        float gmax = 0.f;
        if (s_begin < s_end) {
            float4v gs[NV];
            load_row(gs, grad_out + (int64_t)A.pos_sorted[s_begin] * D);
#pragma unroll
            for (int v = 0; v < NV; ++v) gmax = fmaxf(fmaxf(gmax, fmaxf(fabsf(gs[v].x), fabsf(gs[v].y))), fmaxf(fabsf(gs[v].z), fabsf(gs[v].w)));
            gmax = wave_max(gmax);
            if (lane == 0 && gmax > 0.f && gmax < INFINITY) atomicMax(fx_bits, __float_as_uint(gmax));
        }
        __syncthreads();
        const float m = __uint_as_float(*fx_bits);
        fx_on = m > 0.f;
        fx_k = fx_on ? max(-100, min(27 - ilogbf(m), 100)) : 0;
    }
    const float fx_s = ldexpf(1.0f, fx_k), fx_back = ldexpf(1.0f, -fx_k);
    float4v acc[NV];
    int cur = -1;
    // The current run's token row lives in the wave's LDS strip between two flushes; the strip is also where a finished row is
    // turned into 256-byte-contiguous atomic instructions.
    auto strip_read = [&](float4v (&dst)[NV]) {
#pragma unroll
        for (int v = 0; v < NV; ++v) dst[v] = *(const float4v *)(xp + 4 * (lane + 64 * v));
    };
    auto strip_write = [&](const float4v (&src)[NV], float f) {
#pragma unroll
        for (int v = 0; v < NV; ++v) *(float4v *)(xp + 4 * (lane + 64 * v)) = src[v] * f;
    };
    auto flush = [&]() {                                          // acc (scaled) -> strip -> NE atomic wave-instructions of 256 contiguous bytes
        if (cur < 0) return;
        seg_sync(); strip_write(acc, fx_back); seg_sync();
        float *drow = A.d_tok + (int64_t)cur * D;
        float tr[NE];
#pragma unroll
        for (int j = 0; j < NE; ++j) tr[j] = xp[lane + 64 * j];
        if (!PL_ABL(2)) {
#pragma unroll
            for (int j = 0; j < NE; ++j) atomicAdd(drow + lane + 64 * j, tr[j]);
        }
        seg_sync();
    };
    auto new_run = [&](int tok) {                                 // the finished row leaves, this token's row comes into the strip, an empty sum
        flush();
        cur = tok;
        load_row(acc, tok_table + (int64_t)tok * D);
        __builtin_amdgcn_s_waitcnt(0x0f70);                        // vmcnt(0) (gfx9 encoding: vmcnt [3:0] + [15:14]; expcnt, lgkmcnt left alone)
        strip_write(acc, 1.0f);
        seg_sync();
#pragma unroll
        for (int v = 0; v < NV; ++v) acc[v] = float4v{0.f, 0.f, 0.f, 0.f};
    };
    for (int64_t seg0 = s_begin; seg0 < s_end; seg0 += kSeg) {
        const int len = (int)min((int64_t)kSeg, s_end - seg0);
        int vpos = 0, vtok = 0, vpos_hi = 0, vtok_hi = 0;        // places 0..63 and 64..127 of the segment, a lane each
        if (lane < len) { vpos = A.pos_sorted[seg0 + lane]; vtok = A.tok_sorted[seg0 + lane]; }
        if (64 + lane < len) { vpos_hi = A.pos_sorted[seg0 + 64 + lane]; vtok_hi = A.tok_sorted[seg0 + 64 + lane]; }
        auto pos_at = [&](int i) { return i < 64 ? __builtin_amdgcn_readlane(vpos, i) : __builtin_amdgcn_readlane(vpos_hi, i - 64); };
        auto tok_at = [&](int i) { return i < 64 ? __builtin_amdgcn_readlane(vtok, i) : __builtin_amdgcn_readlane(vtok_hi, i - 64); };
        auto g_row = [&](int i) { return grad_out + (int64_t)pos_at(min(i, len - 1)) * D; };
        float4v b_nx[NV], G0[NV], G1[NV];
        int id_cur[NV], idv_n1 = 0;                               // this place's ids per slot of the lane; the next place's, one per lane
        int64_t idraw_n1 = 0;
        // ---- pipeline fill, requests in the order a step leaves them in (ids, byte rows, gradient row): the first step's waits
        //      are counted for the worse of its two predecessors.  Lookahead indices are clamped to the segment's last place, so
        //      every step issues the same vector-memory instructions (a re-read of a row that is in flight anyway).
        if (BYTES) {
            const int64_t r0 = load_ids(pos_at(0));
            idraw_n1 = load_ids(pos_at(min(1, len - 1)));
            idv_n1 = clamp_id(r0);
            spread_ids(idv_n1, id_cur);
            load_byte_rows(b_nx, id_cur);
        }
        load_row(G0, g_row(0));
        auto step = [&](float4v (&gc)[NV], float4v (&gfree)[NV], const int i) {     // gc: this place's gradient row; gfree: where the next place's goes
            const int tok = tok_at(i);
            if (BYTES) spread_ids(idv_n1, id_cur);
            auto rest = [&]() {
                // (1) the raw ids two places ahead (addresses from a scalar position: depend on nothing in flight)
                int64_t idraw_n2 = 0;
                if (BYTES) idraw_n2 = load_ids(pos_at(min(i + 2, len - 1)));
                // (2) y = a + b_i, then the next place's byte rows go into b's registers (their ids were requested one step ago)
                float4v y[NV];
                strip_read(y);
                if (BYTES) {
#pragma unroll
                    for (int v = 0; v < NV; ++v) y[v] += b_nx[v];
                    int id_n1[NV];
                    idv_n1 = clamp_id(idraw_n1);
                    spread_ids(idv_n1, id_n1);
                    load_byte_rows(b_nx, id_n1);
                    idraw_n1 = idraw_n2;
                }
                // (3) the next place's gradient row
                load_row(gfree, g_row(i + 1));
                // (4) this place
                float ry_s = fx_s, c2_s = 0.f;
                bool finite = true;                                   // wave-uniform: a NaN / infinity anywhere in g or y shows in the two sums
                if (NORM_OUT) {
                    float4v ssv{0.f, 0.f, 0.f, 0.f}, mv{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int v = 0; v < NV; ++v) { ssv += y[v] * y[v]; mv += gc[v] * y[v]; }
                    float ss = (ssv.x + ssv.y) + (ssv.z + ssv.w), m = (mv.x + mv.y) + (mv.z + mv.w);
                    if (!PL_ABL(512)) { ss = wave_sum(ss); m = wave_sum(m); }
                    const float ry = rms_scale(ss, D, A.eps);
                    ry_s = ry * fx_s;
                    c2_s = m * inv_d * ry * ry * ry_s;
                    finite = fabsf(c2_s) < INFINITY && fabsf(ry_s) < INFINITY;
                }
                float amax = 0.f;
                uint32_t abits = 0u;                                  // without the norm: max of the |x| bit patterns (orders NaN above infinity; v_max_f32 drops a NaN)
#pragma unroll
                for (int v = 0; v < NV; ++v) {
                    gc[v] = NORM_OUT ? ry_s * gc[v] - c2_s * y[v] : gc[v] * fx_s;      // dys = 2^k dy
                    acc[v] += gc[v];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (NORM_OUT) amax = fmaxf(amax, fabsf(gc[v][e]));
                        else abits = max(abits, __float_as_uint(gc[v][e]) & 0x7fffffffu);
                    }
                }
                if (!NORM_OUT) amax = abits > 0x7f800000u ? INFINITY : __uint_as_float(abits);
                if (BYTES) {
                    // A lane converts all its NE terms or none: its slots need LDS rows, the workgroup a usable scale, and its largest
                    // |x| must lie in [2^12, 2^31) (or be zero: nothing to add).  The absolute rounding error of a converted term is
                    // <= 2^-(k+1), i.e. 2^-28 of the sampled maximum; a lane whose largest term is 2^-15 of that maximum or less
                    // (rows far below the sample: masked or down-weighted positions) keeps full relative precision through the
                    // float atomics.
                    int sa[NV];
                    bool rows = true;
#pragma unroll
                    for (int v = 0; v < NV; ++v) { sa[v] = byte_slot(id_cur[v]); rows &= sa[v] >= 0; }
                    const bool conv = fx_on && finite && amax < 0x1p31f && amax >= 0x1p12f;
                    const bool ok = (finite && amax == 0.f) || (conv && rows);
                    if (PL_ABL(1)) {
                        if (amax == 123.456f) dbyte_q[lane] = 1;
                    } else if (__all(ok)) {
#pragma unroll
                        for (int v = 0; v < NV; ++v) {
                            unsigned long long *rq = dbyte_q + (size_t)max(sa[v], 0) * qs + wo[v];
#pragma unroll
                            for (int e = 0; e < 4; ++e) atomicAdd(rq + e, (unsigned long long)(long long)__float2int_rn(gc[v][e]));
                        }
                    } else {
                        // rare (a byte id without an LDS row, a term that does not convert): the lane's terms go through its part of the
                        // wave's LDS strip, one at a time, so that this path costs the common one no registers; the token row the strip
                        // held is fetched again afterwards
                        seg_sync(); strip_write(gc, 1.0f); seg_sync();
#pragma unroll
                        for (int v = 0; v < NV; ++v) {
                            const bool lds_ok = conv && sa[v] >= 0;
                            unsigned long long *rq = dbyte_q + (size_t)max(sa[v], 0) * qs + wo[v];
                            float *gq = A.d_byte + (int64_t)id_cur[v] * A.Db + wo[v];
#pragma unroll 1
                            for (int e = 0; e < 4; ++e) {
                                const float x = xp[4 * (lane + 64 * v) + e];
                                if (lds_ok) atomicAdd(rq + e, (unsigned long long)(long long)__float2int_rn(x));
                                else if (x != 0.f) atomicAdd(gq + e, x * fx_back);   // (NaN != 0: it is added)
                            }
                        }
                        seg_sync();
                        load_row(y, tok_table + (int64_t)cur * D);
                        __builtin_amdgcn_s_waitcnt(0x0f70);
                        strip_write(y, 1.0f);
                        seg_sync();
                    }
                }
            };
            // A new run is the only conditional vector-memory work of a step, and it ends with everything this wave has in flight
            // drained; each path then runs its OWN copy of the rest of the step (see the header: waits are counted per path).
            if (tok != cur) { new_run(tok); __builtin_amdgcn_sched_barrier(0); rest(); } else { rest(); }
        };
        int i = 0;
        for (; i + 1 < len; i += 2) {   // two row buffers as register names
            step(G0, G1, i);
            step(G1, G0, i + 1);
        }
        if (i < len) step(G0, G1, i);
    }
    flush();
    if (BYTES) {
        __syncthreads();
        for (int i = tid; i < A.priv_rows * A.Db; i += kPlThreads) {
            const int sl_ = i / A.Db, wi = i - sl_ * A.Db;
            const long long q = (long long)dbyte_q[sl_ * qs + wi];
            if (q == 0) continue;
            const int row = sl_ < A.priv_lo ? sl_ : sl_ - A.priv_lo + A.priv_hi0;
            atomicAdd(A.d_byte + row * A.Db + wi, (float)ldexp((double)q, -fx_k));
        }
    }
#undef PL_ABL
}

// the configuration this kernel is for: SUM / NOOP over full rows of 256, 512 or 768 columns (D = 64 NE, a lane's chunks are four
// elements), one id tensor, no per-embedding norm, no learned scalars; fp32 or bf16 tables and gradient rows
template <int MODE>
static bool plain_layout(const BwdArgs &A) {
    if ((A.D & 255) || A.D > 768 || A.Dt != A.D || A.tok_lo != 0) return false;
    if (MODE == MOT_MIX_SUM && (A.byte_lo != 0 || A.nbk != A.D)) return false;
    if (A.norm_tok || A.norm_byte || A.scale_tok || A.scale_byte || A.d_scale_tok || A.d_scale_byte || A.ids_b || A.g_ld || A.no_tok || A.slot0) return false;
    if (MODE == MOT_MIX_SUM && ((A.Db & 3) || A.Db > 128)) return false;   // a chunk of a row lies inside one byte slot; wide byte rows
                                                                            // (the D-wide "slot" of the cross-attention mixin's two-id backward) do
                                                                            // not fit LDS, and this kernel's path for rows without an LDS slot is slow
    return true;
}

template <int MODE, int NE, bool NORM_OUT, typename T>
static int launch_bwd_plain_t(const BwdArgs &A, size_t lds, hipStream_t stream) {
    const int64_t blocks = (A.n_tokens + 16 * kPlWaves - 1) / (16 * kPlWaves);   // >= 16 sorted positions per wave
    return launch_scatter<embed_mix_bwd_plain_kernel<MODE, NE, NORM_OUT, T>>(A, lds, stream, kPlThreads, blocks, "embed_mix_bwd_plain_kernel");
}
template <int MODE, int NE>
static int launch_bwd_plain(const BwdArgs &A, size_t lds, hipStream_t stream) {
    if (A.in_bf16) {
        if (A.norm_out) return launch_bwd_plain_t<MODE, NE, true, __bf16>(A, lds, stream);
        return launch_bwd_plain_t<MODE, NE, false, __bf16>(A, lds, stream);
    }
    if (A.norm_out) return launch_bwd_plain_t<MODE, NE, true, float>(A, lds, stream);
    return launch_bwd_plain_t<MODE, NE, false, float>(A, lds, stream);
}

template <int MODE>
static int dispatch_ne_plain(const BwdArgs &A, size_t lds, hipStream_t stream) {
    switch (A.D / 64) {
        case 4: return launch_bwd_plain<MODE, 4>(A, lds, stream);
        case 8: return launch_bwd_plain<MODE, 8>(A, lds, stream);
        default: return launch_bwd_plain<MODE, 12>(A, lds, stream);
    }
}

template <int MODE, int NE>
static int launch_bwd(const BwdArgs &A, size_t lds, hipStream_t stream) {
    const int64_t blocks = ((A.n_tokens + kWindow - 1) / kWindow + kBwdWaves - 1) / kBwdWaves;   // one window of sorted positions per wave
    return launch_scatter<embed_mix_bwd_kernel<MODE, NE>>(A, lds, stream, kBwdThreads, blocks, "embed_mix_bwd_kernel");
}

template <int MODE, int NE, bool BF>
static int launch_bwd_full_t(const BwdArgs &A, size_t lds, hipStream_t stream) {
    const int64_t blocks = (A.n_tokens + 16 * kBwdWaves - 1) / (16 * kBwdWaves);   // >= 16 sorted positions per wave
    return launch_scatter<embed_mix_bwd_full_kernel<MODE, NE, BF>>(A, lds, stream, kBwdThreads, blocks, "embed_mix_bwd_full_kernel");
}

template <int MODE, int NE>
static int launch_bwd_full(const BwdArgs &A, size_t lds, hipStream_t stream) {
    if constexpr (!split_row(MODE)) {
        if (A.in_bf16) return launch_bwd_full_t<MODE, NE, true>(A, lds, stream);
    } else if (A.in_bf16) {   // (full_layout sends bf16 split rows to the general kernel)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd: the split-row scatter of this kernel takes fp32 operands");
    }
    return launch_bwd_full_t<MODE, NE, false>(A, lds, stream);
}

// rows that are "full" (see embed_mix_bwd_full_kernel): SUM / NOOP, D a multiple of 64 with a built NE
template <int MODE>
static bool full_layout(const BwdArgs &A) {
    if (A.D & 63) return false;
    if (split_row(MODE)) {   // split row: every 64-element chunk wholly token part or wholly byte part
        if ((A.Dt & 63) || (A.tok_lo & 63) || (A.byte_lo & 63) || (A.nbk & 63) || A.Dt + A.nbk != A.D || A.Db > 0xffff || A.in_bf16) return false;
    } else {
        if (A.Dt != A.D || A.tok_lo != 0) return false;
        if (MODE == MOT_MIX_SUM && (A.byte_lo != 0 || A.nbk != A.D || A.Db > 0xffff)) return false;
        if (A.in_bf16 && ((A.D & 127) || (MODE == MOT_MIX_SUM && (A.Db & 1)))) return false;   // bf16 rows are read as pairs
    }
    if (A.abl & 4) return false;   // abl 4: dev switch back to the general kernel
    const int ne = A.D / 64;
    return ne == 1 || ne == 2 || ne == 4 || ne == 8 || ne == 12 || ne == 16 || ne == 24 || ne == 32;
}

template <int MODE>
static int dispatch_ne_full(const BwdArgs &A, size_t lds, hipStream_t stream) {
    switch (A.D / 64) {
        case 1: return launch_bwd_full<MODE, 1>(A, lds, stream);
        case 2: return launch_bwd_full<MODE, 2>(A, lds, stream);
        case 4: return launch_bwd_full<MODE, 4>(A, lds, stream);
        case 8: return launch_bwd_full<MODE, 8>(A, lds, stream);
        case 12: return launch_bwd_full<MODE, 12>(A, lds, stream);
        case 16: return launch_bwd_full<MODE, 16>(A, lds, stream);
        case 24: return launch_bwd_full<MODE, 24>(A, lds, stream);
        default: return launch_bwd_full<MODE, 32>(A, lds, stream);
    }
}

template <int MODE>
static int dispatch_ne(const BwdArgs &A, size_t lds, hipStream_t stream) {
    const int ne = (A.D + 63) / 64;
    if (ne <= 1) return launch_bwd<MODE, 1>(A, lds, stream);
    if (ne <= 2) return launch_bwd<MODE, 2>(A, lds, stream);
    if (ne <= 4) return launch_bwd<MODE, 4>(A, lds, stream);
    if (ne <= 8) return launch_bwd<MODE, 8>(A, lds, stream);
    if (ne <= 12) return launch_bwd<MODE, 12>(A, lds, stream);
    if (ne <= 16) return launch_bwd<MODE, 16>(A, lds, stream);
    if (ne <= 24) return launch_bwd<MODE, 24>(A, lds, stream);
    if (ne <= 32) return launch_bwd<MODE, 32>(A, lds, stream);
    return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd: model_dim %d > 2048 is not built", A.D);
}

// ------------------------------------------------------------------------------------------
// scatter stage shared by all modes: sort the positions by token id (launch_group_positions, mot_group.hip), then embed_mix_bwd_kernel.
// `ws_ints` = [counts: tok_rows][starts: tok_rows][rank: N][pos_sorted: N][tok_sorted: N] (int32).
// ------------------------------------------------------------------------------------------
size_t scatter_ws_ints(const MotEmbedMixDesc &d) { return 2 * (size_t)d.tok_rows + 3 * (size_t)(d.n_rows * d.tokens_per_row); }

template <int MODE>
static int run_scatter(BwdArgs &A, const MotEmbedMixDesc &d, int32_t *ws_ints, float *rnorm_ws, hipStream_t stream) {
    int rc;
    A.abl = 0;
#ifdef MOT_DEV_ABLATION
    if (getenv("MOT_BWD_ABL")) A.abl = atoi(getenv("MOT_BWD_ABL"));
#endif
    if (d.tok_rows >= (1 << 21) - 1)   // (token << 11 | index) of bwd_rank_kernel must stay below its 0xffffffff padding key
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd: token tables of %lld rows (>= 2^21 - 1) are not built", (long long)d.tok_rows);
    const bool full = full_layout<MODE>(A) && !A.g_ld;   // (a row stride is known to the lane-contiguous kernel and to the general one)
    bool lc = false, plain = false;
    if constexpr (!split_row(MODE)) {
        lc = lc_layout<MODE>(A) && !(A.abl & 8);   // abl 8: dev switch back to the strided kernels
        plain = plain_layout<MODE>(A) && !(A.abl & 24);   // abl 16: dev switch back to the general kernels
        lc = lc || plain;                           // (LDS layout below: one fp32 row per wave, byte-table rows padded by one sum)
    }
    // LDS besides the privatised byte-table sums: per-wave per-slot accumulators (strided kernels) or per-wave transposition rows (lane-contiguous)
    size_t lds = lc ? (size_t)(plain ? kPlWaves : kLcWaves) * A.D * sizeof(float) + 16 : 2 * (size_t)kBwdWaves * kMaxBpt * sizeof(float) + 16;
    // the positions grouped by token id: given by the caller (mot_token_order, same layout as the workspace) or made here
    if (A.pos_sorted == nullptr || A.tok_sorted == nullptr)
        if ((rc = launch_group_positions(A.tokens, A.n_tokens, A.tok_rows, ws_ints, &A.pos_sorted, &A.tok_sorted, A.status, stream))) return rc;
#ifdef MOT_DEV_ABLATION
    if (getenv("MOT_BWD_SORT_ONLY")) return MOT_OK;  // dev: inspect the sort prologue's workspace from the host
#endif
    A.priv_lo = 0; A.priv_hi0 = (int)d.byte_rows; A.priv_rows = 0;
    if (MODE != MOT_MIX_NOOP) {
        // as many byte-table rows as 150 KiB of LDS hold at 8 bytes per element; when not all fit, the last 32 rows
        // (pad / eot and other specials sit at the end of the byte vocabulary) and the first cap-32
        const size_t row_q = (size_t)d.byte_dim + (lc ? 1 : 0);   // the lane-contiguous kernel pads its rows by one sum
        const int64_t cap = (int64_t)((150 * 1024 - lds) / (row_q * 8));
        if (cap >= d.byte_rows) { A.priv_lo = (int)d.byte_rows; A.priv_rows = (int)d.byte_rows; }
        else if (cap > 64) { A.priv_lo = (int)cap - 32; A.priv_hi0 = (int)d.byte_rows - 32; A.priv_rows = (int)cap; }
        lds += (size_t)A.priv_rows * row_q * 8 + 8;
        if (d.norm_byte && !(split_row(MODE) && d.ids_b)) {
            rc = launch_rows_rnorm(A.byte_table, d.byte_rows, d.byte_dim, A.eps, rnorm_ws, A.in_bf16 ? MOT_BF16 : MOT_F32, stream);
            if (rc) return rc;
            A.byte_rnorm = rnorm_ws;
        }
    }
    if constexpr (!split_row(MODE)) {
        if (plain) return dispatch_ne_plain<MODE>(A, lds, stream);
        if (lc) return dispatch_ne_lc<MODE>(A, lds, stream);
    }
    if (full) return dispatch_ne_full<MODE>(A, lds, stream);
    return dispatch_ne<MODE>(A, lds, stream);
}

// what the other backward units see of the scatter (mot_bwd.hpp): the kernels are instantiated in this unit only
int run_scatter(int mode, BwdArgs &A, const MotEmbedMixDesc &d, int32_t *ws_ints, float *rnorm_ws, hipStream_t stream) {
    switch (mode) {
        case MOT_MIX_SUM: return run_scatter<MOT_MIX_SUM>(A, d, ws_ints, rnorm_ws, stream);
        case MOT_MIX_CONCAT_LINEAR: return run_scatter<MOT_MIX_CONCAT_LINEAR>(A, d, ws_ints, rnorm_ws, stream);
        case MOT_MIX_CONCAT: return run_scatter<MOT_MIX_CONCAT>(A, d, ws_ints, rnorm_ws, stream);
        default: return run_scatter<MOT_MIX_NOOP>(A, d, ws_ints, rnorm_ws, stream);
    }
}
bool lc_layout(int mode, const BwdArgs &A) { return mode == MOT_MIX_SUM ? lc_layout<MOT_MIX_SUM>(A) : lc_layout<MOT_MIX_NOOP>(A); }

void fill_bwd_args(BwdArgs &A, const MotEmbedMixDesc &d, const MotEmbedMixGrads &gr) {
    A.tokens = d.tokens; A.n_tokens = d.n_rows * d.tokens_per_row; A.bpt = d.bpt;
    A.ids_a = d.ids_a; A.ids_b = d.ids_b;
    A.tok_table = (const float *)d.tok_table; A.tok_rows = d.tok_rows; A.D = d.tok_dim;
    A.byte_table = (const float *)d.byte_table; A.byte_rows = d.byte_rows; A.Db = d.byte_dim;
    A.norm_tok = d.norm_tok; A.norm_byte = d.norm_byte; A.norm_out = d.norm_out;
    A.in_bf16 = d.dtype == MOT_BF16;
    A.eps = d.eps > 0.f ? d.eps : (A.in_bf16 ? kBf16Eps : FLT_EPSILON);
    A.scale_tok = d.scale_tok; A.scale_byte = d.scale_byte; A.byte_rnorm = nullptr;
    A.grad_out = (const float *)gr.grad_out;
    A.d_tok = (float *)gr.d_tok_table; A.d_byte = (float *)gr.d_byte_table;
    A.d_scale_tok = gr.d_scale_tok; A.d_scale_byte = gr.d_scale_byte;
    A.status = d.status;
    A.pos_sorted = A.tok_sorted = nullptr;
    A.g_ld = 0; A.no_tok = 0; A.slot0 = 0;
    if (gr.token_order) {   // [counts: rows][starts: rows][rank: n][pos_sorted: n][tok_sorted: n], as launch_group_positions lays it out
        const int64_t n = d.n_rows * d.tokens_per_row;
        A.pos_sorted = gr.token_order + 2 * d.tok_rows + n;
        A.tok_sorted = A.pos_sorted + n;
    }
    A.Dt = d.tok_dim; A.tok_lo = 0; A.byte_lo = 0; A.nbk = d.bpt * d.byte_dim;
    if (d.mode == MOT_MIX_CONCAT) { A.D = d.tok_dim + A.nbk; A.byte_lo = d.tok_dim; }   // the row is cat(token row, byte rows)
}

static size_t bwd_rnorm_floats(const MotEmbedMixDesc &d) { return mixes_bytes(d.mode) ? ((size_t)d.byte_rows + 3) & ~(size_t)3 : 0; }
size_t embed_mix_bwd_workspace_bytes(const MotEmbedMixDesc &d) {
    if (d.mode == MOT_MIX_MEAN) return embed_mix_bwd_mean_workspace_bytes(d);
    if (d.mode == MOT_MIX_CONCAT_LINEAR) return embed_mix_bwd_linear_workspace_bytes(d);
    return (bwd_rnorm_floats(d) + scatter_ws_ints(d)) * 4;
}

int launch_embed_mix_bwd(const MotEmbedMixDesc &d, const MotEmbedMixGrads &gr, hipStream_t stream) {
    if (d.n_rows * d.tokens_per_row > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd: more than 2^31 tokens");
    if (d.mode == MOT_MIX_CONCAT_LINEAR) return launch_embed_mix_bwd_linear(d, gr, stream);
    if (d.mode == MOT_MIX_MEAN) return launch_embed_mix_bwd_mean(d, gr, stream);
    if (mixes_bytes(d.mode) && d.id_source != MOT_IDS_GIVEN)
        return set_error(MOT_EUNSUPPORTED, "embed_mix_bwd: pass the byte ids the forward returned (MOT_IDS_GIVEN)");
    BwdArgs A;
    fill_bwd_args(A, d, gr);
    const size_t need = embed_mix_bwd_workspace_bytes(d);
    if (!d.workspace || d.workspace_bytes < need)
        return set_error(MOT_EWORKSPACE, "embed_mix_bwd: needs %zu workspace bytes, got %zu", need, d.workspace_bytes);
    float *rn = (float *)d.workspace;
    int32_t *ints = (int32_t *)(rn + bwd_rnorm_floats(d));
    return run_scatter(d.mode, A, d, ints, rn, stream);
}

}  // namespace mot
