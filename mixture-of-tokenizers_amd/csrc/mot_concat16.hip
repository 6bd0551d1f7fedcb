// mot_concat16.hip -- the concat + linear mixin in the production dtype as ONE dense-MFMA kernel (gfx950):
//     x = rms_norm?( bf16( W . cat(norm?(E_t[tok]), norm?(E_b[id_0]), ..., norm?(E_b[id_{bpt-1}])) + bias ) )
// (ByteMixinConcat on FlexibleEmbedding's outputs, scaled-pre-train/train_gpt.py:342-379, 430-443, CastedLinear 185-186;
//  DigitMixinConcat, mathblations/model.py:256-268), bf16 tables / weight / output, fp32 accumulation.
//
// The composed path (index kernels -> concat_rows_kernel -> gemm_rows_bf16_kernel -> rows_finish_kernel) spends 40 % of
// its time outside the contraction and runs the contraction itself at 23 % of the bf16 MFMA peak: 128 x 128 blocks read one
// 16-byte LDS fragment per MFMA, and the concat operand makes two trips through HBM.  Here
//   * a workgroup owns WHOLE output rows (64 MT tokens x all Dm = 128 NT columns; 8 waves as 2 x 4, a wave 32 MT x 32 NT), so
//     the row norm is an epilogue, and a fragment feeds MT or NT MFMAs;
//   * the A operand is GATHERED: per 32-deep step a thread fetches one 16-byte piece of a token row or byte row, scales it by
//     the row's rms factor, rounds to bf16 (the reference's rounding point: norm() returns a bf16 tensor) and writes it into the
//     step's LDS tile -- the concat tensor never exists;
//   * W is staged by LDS-DMA (global_load_lds, 16 bytes per lane, no staging registers) into NS stages, XOR-swizzled on the
//     SOURCE side so that the lane-linear LDS image reads back without bank conflicts: piece p of row n sits at
//     n * 64 + ((p ^ (n >> 2)) & 3) * 16;
//   * the output tile leaves through LDS (the W stages, free by then) as whole 16-byte pieces: a lane holds NT consecutive outputs
//     of a row (the stage rows of W are permuted for that), 32 lanes then take a row, sum its squares, scale and store.
// Two barriers per step (the gathered tile is single-buffered: LDS is full); the DMA of steps s + 1 and s + 2 and the gathered
// pieces of steps s + 1 and s + 2 are in flight while step s multiplies; every wait in the loop is counted (see the step).
#include "mot_wave.hpp"
#include <type_traits>
// (clang wants the explicit captures below for operands of inline asm inside generic lambdas, and then calls them unused)
#pragma clang diagnostic ignored "-Wunused-lambda-capture"

namespace mot {

typedef __bf16 bf16x8c __attribute__((ext_vector_type(8)));
typedef float f32x16c __attribute__((ext_vector_type(16)));

struct C16Args {
    const int32_t *tokens;     // [n]
    const int64_t *ids;        // [n, bpt] as the reference's loader emits them, or
    const uint16_t *ids16;     // [n, bpt] compact and range-checked, from wave_ids16_kernel (ids pulled from the token->byte table)
    int64_t n;
    const __bf16 *tok_table; int64_t tok_rows; int Dt;
    const __bf16 *byte_table; int64_t byte_rows; int Db; int bpt;
    int norm_tok;              // token rows are rms-normalised (factor computed per tile, below)
    const float *byte_rnorm;   // [byte_rows] rms factors of the byte table, or null: no byte norm, or
    int norm_byte_here;        // the workgroups compute the factors themselves (tables of up to kC16NormHere rows)
    const __bf16 *W;           // [Dm, K]
    const __bf16 *bias;        // [Dm] or null
    int K, Dm, tok_lo, byte_lo;
    int norm_out;
    float eps;
    __bf16 *out;               // [n, Dm]
    float *row_rnorm;          // optional [n]
    uint32_t *status;
};

constexpr int kC16Threads = 512;
constexpr int kC16NormHere = 1024;
#ifdef C16_STAMPS   // dev: wall-clock stamps (10 ns units) of workgroup phases, printed once by the launcher
__device__ unsigned long long c16_stamps[4096 * 8];
#define C16_STAMP(i) do { if (threadIdx.x == 0 && blockIdx.x < 4096) c16_stamps[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define C16_STAMP(i) do {} while (0)
#endif
typedef int i32x4c __attribute__((ext_vector_type(4)));

// LDS reads the COMPILER must not see.  hipcc orders every LDS read it emits behind every LDS-DMA still in flight (it cannot
// tell which bytes the DMA writes), i.e. s_waitcnt vmcnt(0) in front of the first ds_read after a global_load_lds -- which
// would serialise the DMA of step s + 2 with the multiplies of step s.  The reads of the loop are therefore inline asm, ordered
// against the DMA by hand: a stage is read only after the barrier behind the wait that retired it (see the loop).
#define C16_FRAG(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
__device__ __forceinline__ uint32_t lds_off(const void *p) { return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char *)p; }
__device__ __forceinline__ uint32_t lds_u16_now(uint32_t addr) {
    uint32_t v;
    asm volatile("ds_read_u16 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ float lds_f32_now(uint32_t addr) {
    float v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}
// workgroup barrier that waits for this wave's LDS traffic only (no vmcnt drain: the DMA and the gathered pieces stay in flight)
__device__ __forceinline__ void c16_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// NS stages of W in LDS (NS - 1 steps of DMA in flight), ONE stage of the gathered operand (its next step waits in registers)
#define C16_PASS_BEGIN for (int hh = 0; hh < NH; ++hh) {
#define C16_PASS_END }
// NH: column passes.  model_dim 1024 does not fit a 128-token tile's accumulators (256 registers); as 64-token tiles it streamed all
// of W per 64 tokens and paid 8 DMA instructions per 16 MFMAs.  NH = 2 keeps the 128-token tile and computes its columns in two
// passes of 512 (the tile's ids, rms factors and token-row norms are made once; the gathered operand is walked twice, out of L2):
// pass 0 stores y un-normalised and keeps each row's sum of squares, pass 1 completes the sum, stores its half normalised and
// rescales the first half in place (every lane re-reads exactly the pieces it wrote).
// RES: the residual form for the linear-on-bytes mixin (mot_bytefc.hip, runs/71051_*.py:225-229), x = norm(tok + W . cat(bytes)): the
// caller passes Dt = 0, so the K loop walks the byte part only and the token row never enters the contraction; it is added in the
// epilogue's row pass instead, where 32 lanes hold a row in 16-byte pieces -- after the product was rounded to bf16, and the sum is
// rounded before the squares are taken (the reference's bf16 tensors: F.linear's result, the add).  Rows are Dm wide there.
template <int MT, int NT, int NS, int NH = 1, bool RES = false>
__global__ __launch_bounds__(kC16Threads) void concat16_gemm_kernel(const C16Args P) {
#include "mot_concat16_body.inc"
}

// The same workgroup program over a (token tile, slot) grid: slot blockIdx.y brings its own tables, W and outputs; the tokens, the
// ids and every shape are shared (the mixture-of-tokenizers value embeddings, mot_valuemix.hip: ONE launch for all slots).
struct C16SlotArgs {
    C16Args base;
    const __bf16 *tok_table[4], *byte_table[4], *W[4];
    __bf16 *out[4];
    float *row_rnorm[4];
};
template <int MT, int NT, int NS, int NH>
__global__ __launch_bounds__(kC16Threads) void concat16_slots_kernel(const C16SlotArgs S) {
    constexpr bool RES = false;
    const C16Args P = [&] {
        C16Args Q = S.base;
        const int j = blockIdx.y;
        Q.tok_table = S.tok_table[j]; Q.byte_table = S.byte_table[j]; Q.W = S.W[j]; Q.out = S.out[j]; Q.row_rnorm = S.row_rnorm[j];
        return Q;
    }();
#include "mot_concat16_body.inc"
}

static size_t c16_lds_base(int MT, int NT, int NS, int bpt);
template <int MT, int NT, int NS, int NH = 1, bool RES = false>
static int launch_c16(const C16Args &P0, hipStream_t stream) {
    constexpr int BM = 64 * MT;
    const C16Args &P = P0;
    const size_t lds = c16_lds_base(MT, NT, NS, P.bpt) + (size_t)P.byte_rows * 4 + (NH > 1 ? BM * 4 : 0);
    if (lds > 160 * 1024) return set_error(MOT_EUNSUPPORTED, "concat16: needs %zu B of LDS", lds);
    static std::atomic<uint64_t> ok{0};
    if (int rc = ensure_max_dyn_lds((const void *)concat16_gemm_kernel<MT, NT, NS, NH, RES>, ok, "concat16_gemm_kernel")) return rc;
    const int64_t blocks = (P.n + BM - 1) / BM;
    if (blocks > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "concat16: too many rows");
    hipLaunchKernelGGL((concat16_gemm_kernel<MT, NT, NS, NH, RES>), dim3((unsigned)blocks), dim3(kC16Threads), lds, stream, P);
#ifdef C16_STAMPS
    static int calls = 0;
    if (++calls == 60) {
        static unsigned long long h[4096 * 8];
        hipDeviceSynchronize();
        hipMemcpyFromSymbol(h, HIP_SYMBOL(c16_stamps), sizeof(h));
        const int nb = (int)(blocks < 4096 ? blocks : 4096);
        unsigned long long t0 = ~0ull;
        for (int b = 0; b < nb; ++b) t0 = h[b * 8] < t0 ? h[b * 8] : t0;
        double sum[8] = {0}, mx[8] = {0};
        for (int b = 0; b < nb; ++b)
            for (int i = 0; i < 8; ++i) { const double v = (double)(h[b * 8 + i] - t0) * 0.01; sum[i] += v; mx[i] = v > mx[i] ? v : mx[i]; }
        fprintf(stderr, "c16 stamps (us since first start; mean / max over %d workgroups):", nb);
        for (int i = 0; i < 8; ++i) fprintf(stderr, "  [%d] %.1f/%.1f", i, sum[i] / nb, mx[i]);
        fprintf(stderr, "\n  first-round groups only (start < 2 us):");
        double s2[8] = {0}; int n2 = 0;
        for (int b = 0; b < nb; ++b) if ((h[b * 8] - t0) < 200) { ++n2; for (int i = 0; i < 8; ++i) s2[i] += (double)(h[b * 8 + i] - t0) * 0.01; }
        for (int i = 0; i < 8; ++i) fprintf(stderr, "  [%d] %.1f", i, s2[i] / (n2 ? n2 : 1));
        fprintf(stderr, "  (%d groups)\n", n2);
    }
#endif
    return check_launch("concat16_gemm_kernel");
}

// ------------------------------------------------------------------------------------------ ids pulled from the token->byte table
// The byte-index work of the loader (tokens_to_bytes + pull, data_creation.py:60-76, 79-176, 179-305) for the gather-GEMM above:
// the wave-local indexer of the fused SUM kernel (mot_wave.hpp: a unit of 16 or 32 tokens per wave, its 64-token window, halo walk
// across the window's edge) writes the pulled ids ONCE, as 16-bit values (2 bytes per slot instead of the two int64 tensors the
// separate index kernels write and read back: 2 MB instead of 2 x 8 + 8 MB at 65 536 tokens), range-checked, plus the int64 parity
// outputs and the pad statistics when the caller asked for them.
// tokens per wave: 32 (7.2 us at 65 536 tokens; 9.0 with 16, 13.4 with 8: fewer windows to build); 16 for small batches
static int ids16_unit(int64_t n) { return n >= 16384 ? 32 : 16; }
template <int DIR, typename E>
__global__ __launch_bounds__(kThreads) void wave_ids16_kernel(const MixArgs A, uint16_t *__restrict__ ids16) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_wave[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t unit_id = (int64_t)blockIdx.x * kWaves + wave;
    if (unit_id >= A.n_units) return;             // no workgroup barrier below: a wave may leave on its own
    const int64_t row = unit_id / A.units_per_row;
    const int64_t u0 = (unit_id - row * A.units_per_row) * A.unit;
    const int ntok = (int)min((int64_t)A.unit, A.T - u0);
    const WaveLds W = wave_lds_carve(lds_wave + (size_t)wave * A.wave_lds, A.unit, A.bpt, false, DIR != kPullNone ? (int)sizeof(E) : 0);
    WaveIndexer<DIR, E> ix(A, W, row, u0, ntok, false);
    ix.tokens();
    ix.load_rows();
    ix.finish();
    const int bpt = A.bpt, sv = bpt | 1, n = ntok * bpt;
    uint16_t *dst = ids16 + (row * A.T + u0) * bpt;
    const float inv = 1.0f / (float)bpt;
    for (int i = lane; i < n; i += 64) {
        const int t = __float2int_rd(((float)i + 0.5f) * inv);     // i / bpt, exact for i < 2^22
        dst[i] = (uint16_t)W.ids[t * sv + (i - t * bpt)];
    }
}

int launch_wave_ids16(const MotEmbedMixDesc &d, uint16_t *ids16, hipStream_t stream) {
    MixArgs A;
    fill_mix_args(A, d);
    A.unit = ids16_unit(d.n_rows * d.tokens_per_row);
    A.units_per_row = (d.tokens_per_row + A.unit - 1) / A.unit;
    A.n_units = d.n_rows * A.units_per_row;
    const int64_t blocks = (A.n_units + kWaves - 1) / kWaves;
    if (blocks > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "concat16: too many units");
    if (blocks == 0) return MOT_OK;
    A.wave_lds = (int)wave_lds_bytes(A.unit, d.bpt, false, d.pull_dir != MOT_PULL_NONE ? d.ttb_elem_bytes : 0);
    const size_t lds = (size_t)A.wave_lds * kWaves;
    if (lds > 64 * 1024) return set_error(MOT_EUNSUPPORTED, "concat16: the index pass needs %zu B of LDS", lds);
#define MOT_IDS16_LAUNCH(DIR, E) hipLaunchKernelGGL((wave_ids16_kernel<DIR, E>), dim3((unsigned)blocks), dim3(kThreads), lds, stream, A, ids16)
    if (d.ttb_elem_bytes == 2) {
        if (d.pull_dir == MOT_PULL_LEFT) MOT_IDS16_LAUNCH(kPullLeft, int16_t);
        else if (d.pull_dir == MOT_PULL_RIGHT) MOT_IDS16_LAUNCH(kPullRight, int16_t);
        else MOT_IDS16_LAUNCH(kPullNone, int16_t);
    } else {
        if (d.pull_dir == MOT_PULL_LEFT) MOT_IDS16_LAUNCH(kPullLeft, int32_t);
        else if (d.pull_dir == MOT_PULL_RIGHT) MOT_IDS16_LAUNCH(kPullRight, int32_t);
        else MOT_IDS16_LAUNCH(kPullNone, int32_t);
    }
#undef MOT_IDS16_LAUNCH
    return check_launch("wave_ids16_kernel");
}

static size_t c16_lds_base(int MT, int NT, int NS, int bpt) {
    return (size_t)NS * 128 * NT * 64 + (size_t)64 * MT * 64 + (((size_t)64 * MT * bpt * 2 + 15) & ~(size_t)15);
}
struct C16Shape { int MT, NT, NS, NH; };
static bool c16_two_pass() {   // model_dim 1024 as two column passes of a 128-token tile (dev builds can switch back to 64-token tiles)
#ifdef MOT_DEV_ABLATION
    if (getenv("MOT_C16_1024_OLD")) return false;
#endif
    return true;
}
static C16Shape c16_shape(int Dm) {
    switch (Dm) {
        case 256: return {2, 2, 3, 1};
        case 512: return {2, 4, 3, 1};
        case 768: return {2, 6, 3, 1};
        default: return c16_two_pass() ? C16Shape{2, 4, 3, 2} : C16Shape{1, 8, 2, 1};   // 1024
    }
}

// the shapes this kernel takes: bf16, one id tensor, pieces of 8 elements that never straddle a part (Dt, Db multiples of 8),
// whole 32-deep steps, model_dim = 128 NT with an accumulator tile that fits (NT <= 6 at 128-token tiles, 8 at 64-token tiles),
// 16-bit byte ids, and the tile's ids and the byte rows' rms factors beside the stages in LDS
bool concat16_norm_in_kernel(const MotEmbedMixDesc &d) { return d.byte_rows <= kC16NormHere; }
bool concat16_usable(const MotEmbedMixDesc &d) {
    if (d.dtype != MOT_BF16 || d.ids_b || d.scale_tok || d.scale_byte || d.bpt < 1) return false;
    const int K = d.tok_dim + d.bpt * d.byte_dim;
    if ((d.tok_dim & 7) || (d.byte_dim & 7) || (K & 31) || d.byte_rows > 65536) return false;
    const int Dm = d.model_dim;
    if (Dm != 256 && Dm != 512 && Dm != 768 && Dm != 1024) return false;
    if (((uintptr_t)d.weight | (uintptr_t)d.tok_table | (uintptr_t)d.byte_table | (uintptr_t)d.out) & 15) return false;
    const C16Shape sh = c16_shape(Dm);
    return c16_lds_base(sh.MT, sh.NT, sh.NS, d.bpt) + (size_t)d.byte_rows * 4 + (sh.NH > 1 ? 64 * sh.MT * 4 : 0) <= 160 * 1024;
}

// the residual form (RES above) takes the same family with the token part out of the contraction: tok_dim == model_dim, K = bpt * byte_dim
bool concat16_residual_usable(const MotEmbedMixDesc &d) {
    if (d.tok_dim != d.model_dim || d.norm_tok || d.norm_byte || d.bias || d.bytes_first) return false;
    MotEmbedMixDesc b = d;
    b.tok_dim = 0;
    return concat16_usable(b);
}

// rn_byte: per-row rms factors of the byte table (launch_rows_rnorm); null when the byte part is not normalised or the table is
// small enough for the workgroups to compute them (concat16_norm_in_kernel)
// residual: d.weight is [model_dim, bpt * byte_dim] and the token row is added behind the product (concat16_residual_usable)
int launch_concat16(const MotEmbedMixDesc &d, const int32_t *tokens, const int64_t *ids, const uint16_t *ids16, int64_t n, const float *rn_byte,
                    void *out, float *row_rnorm, hipStream_t stream, bool residual) {
    C16Args P;
    P.tokens = tokens; P.ids = ids; P.ids16 = ids16; P.n = n;
    P.tok_table = (const __bf16 *)d.tok_table; P.tok_rows = d.tok_rows; P.Dt = d.tok_dim;
    P.byte_table = (const __bf16 *)d.byte_table; P.byte_rows = d.byte_rows; P.Db = d.byte_dim; P.bpt = d.bpt;
    P.norm_tok = d.norm_tok; P.byte_rnorm = rn_byte; P.norm_byte_here = d.norm_byte && !rn_byte;
    P.W = (const __bf16 *)d.weight; P.bias = (const __bf16 *)d.bias;
    P.K = d.tok_dim + d.bpt * d.byte_dim; P.Dm = d.model_dim;
    P.tok_lo = d.bytes_first ? d.bpt * d.byte_dim : 0; P.byte_lo = d.bytes_first ? 0 : d.tok_dim;
    P.norm_out = d.norm_out; P.eps = d.eps > 0.f ? d.eps : kBf16Eps;
    P.out = (__bf16 *)out; P.row_rnorm = d.norm_out ? row_rnorm : nullptr; P.status = d.status;
    if (residual) {
        P.Dt = 0; P.K = d.bpt * d.byte_dim; P.tok_lo = P.byte_lo = 0;
        switch (d.model_dim) {
            case 256: return launch_c16<2, 2, 3, 1, true>(P, stream);
            case 512: return launch_c16<2, 4, 3, 1, true>(P, stream);
            case 768: return launch_c16<2, 6, 3, 1, true>(P, stream);
            default: return launch_c16<2, 4, 3, 2, true>(P, stream);
        }
    }
    switch (d.model_dim) {
        case 256: return launch_c16<2, 2, 3>(P, stream);
        case 512: return launch_c16<2, 4, 3>(P, stream);
        case 768: return launch_c16<2, 6, 3>(P, stream);
        default: return c16_two_pass() ? launch_c16<2, 4, 3, 2>(P, stream) : launch_c16<1, 8, 2>(P, stream);
    }
}

template <int MT, int NT, int NS, int NH>
static int launch_c16_slots(const C16SlotArgs &S, int n_slots, hipStream_t stream) {
    constexpr int BM = 64 * MT;
    const C16Args &P = S.base;
    const size_t lds = c16_lds_base(MT, NT, NS, P.bpt) + (size_t)P.byte_rows * 4 + (NH > 1 ? BM * 4 : 0);
    if (lds > 160 * 1024) return set_error(MOT_EUNSUPPORTED, "concat16: needs %zu B of LDS", lds);
    static std::atomic<uint64_t> ok{0};
    if (int rc = ensure_max_dyn_lds((const void *)concat16_slots_kernel<MT, NT, NS, NH>, ok, "concat16_slots_kernel")) return rc;
    const int64_t blocks = (P.n + BM - 1) / BM;
    if (blocks > 0x7fffffffLL) return set_error(MOT_EUNSUPPORTED, "concat16: too many rows");
    hipLaunchKernelGGL((concat16_slots_kernel<MT, NT, NS, NH>), dim3((unsigned)blocks, (unsigned)n_slots), dim3(kC16Threads), lds, stream, S);
    return check_launch("concat16_slots_kernel");
}

// d describes slot 0 (concat16_usable(d) holds, no input norms, no bias); every slot shares its shapes
int launch_concat16_slots(const MotEmbedMixDesc &d, const Concat16Slots &Q, const int32_t *tokens, const int64_t *ids, int64_t n, hipStream_t stream) {
    if (Q.n < 1 || Q.n > 4) return set_error(MOT_EINVAL, "concat16: %d slots", Q.n);
    C16SlotArgs S{};
    C16Args &P = S.base;
    P.tokens = tokens; P.ids = ids; P.ids16 = nullptr; P.n = n;
    P.tok_rows = d.tok_rows; P.Dt = d.tok_dim; P.byte_rows = d.byte_rows; P.Db = d.byte_dim; P.bpt = d.bpt;
    P.norm_tok = 0; P.byte_rnorm = nullptr; P.norm_byte_here = 0; P.bias = nullptr;
    P.K = d.tok_dim + d.bpt * d.byte_dim; P.Dm = d.model_dim; P.tok_lo = 0; P.byte_lo = d.tok_dim;
    P.norm_out = d.norm_out; P.eps = d.eps > 0.f ? d.eps : kBf16Eps; P.status = d.status;
    for (int j = 0; j < Q.n; ++j) {
        S.tok_table[j] = (const __bf16 *)Q.tok_table[j]; S.byte_table[j] = (const __bf16 *)Q.byte_table[j]; S.W[j] = (const __bf16 *)Q.weight[j];
        S.out[j] = (__bf16 *)Q.out[j]; S.row_rnorm[j] = d.norm_out ? Q.row_rnorm[j] : nullptr;
    }
    switch (d.model_dim) {
        case 256: return launch_c16_slots<2, 2, 3, 1>(S, Q.n, stream);
        case 512: return launch_c16_slots<2, 4, 3, 1>(S, Q.n, stream);
        case 768: return launch_c16_slots<2, 6, 3, 1>(S, Q.n, stream);
        default: return launch_c16_slots<2, 4, 3, 2>(S, Q.n, stream);
    }
}

}  // namespace mot
