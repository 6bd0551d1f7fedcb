// mot_nexttoken.hip -- the generation step behind the plain head: the last position's logits, the top-k and top-p cuts and the draw
// in one call (mot_next_token), nothing read on the host.  Restates inference/inference.py:420-444 (and the print of :448-453):
//   lm_head on the last position / temperature; torch.topk's cut; the cut on a full sort's cumulative softmax; argmax or multinomial.
//
// Two kernels per chunk of rows:
//   nexttoken_skinny   n_rows <= 16: l = T(c x) W^T with W read ONCE in 16-byte vectors.  The rows of x, normed and rounded to the
//                      call's dtype as F.rms_norm's output is in front of lm_head, sit in LDS; a wave owns four class rows at a time,
//                      every lane a 16-byte slice of the reduction, the waves' DPP sums close each product.  Stores fp32 or bf16.
//                      Above 16 rows the same rows of x are written by nexttoken_rows_in and the product is launch_product_nt.
//   nexttoken_row      one workgroup per row, wide_rows' geometry (the row in registers up to eight 16-byte vectors a thread:
//                      32 768 classes in fp32, 65 536 in bf16; read again from L2 above that).
//                      All order decisions are taken on the stored logit's order-preserving integer image (-0 counts as +0):
//                      the k-th largest value and the top-p boundary come from a three-level radix selection (11 + 11 + 10 bits),
//                      each level one LDS histogram of 64-bit integers: counts for top-k, masses for top-p.  No sort, no buffer of
//                      vocab beyond the logits.
// The masses are integers: q = ceil(exp((l - m) / temperature) * 2^44), at least 1 for a finite logit, 0 for -inf, so every sum
// (histogram bins, Z, the draw's running mass) is an integer sum below 2^63 whose value cannot depend on the order of its adds:
// the same bits on every run, with integer LDS atomics and no float atomic anywhere.  The rounding up adds at most vocab * 2^-44
// (1.5e-8 at 262 144 classes) to a Z that is at least 1.
// The draw walks the kept classes in ascending class order: step i of the sweep gives wave w the 64 consecutive vectors
// [(i * waves + w) * 64, +64), so the sums of these spans, in (i, w) order, are the prefix masses of contiguous class spans; one
// wave scans them, the owning wave scans its lanes, the owning lane its vector.
#include "mot_widehead.hpp"

namespace mot {
namespace {

constexpr int kSkinnyRows = 16;       // the skinny product takes up to this many rows
constexpr int kSkinnyThreads = 512, kSkinnyWaves = kSkinnyThreads / 64;
constexpr int kSkinnyCls = 4;         // class rows a wave holds in flight
constexpr int kSkinnyGrid = 1024;
constexpr int kNtBins = 2048;         // bins of a selection level; also bounds the spans of the draw (64 steps x 16 waves)
constexpr int kNtMaxTop = 8;
constexpr float kNtMassScale = 0x1p44f;
constexpr double kNtMassUnit = 0x1p-44;

// ---------------------------------------------------------------------------------------------- the rows of x as the product takes them
// norm_round_row (mot_headrows.hpp): a row, normed (norm_in) and rounded to T; one wave
template <typename T>
__global__ __launch_bounds__(kThreads) void nexttoken_rows_in(const T *__restrict__ x, int64_t x_stride, int64_t n, int K, int norm_in, float eps,
                                                              T *__restrict__ hg) {
    const int64_t j = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (j >= n) return;
    norm_round_row<T>(x + j * x_stride, K, norm_in, eps, hg + j * K);
}

// S[r][v] = T(sum_k xs[r][k] W[v][k]) for r < n_rows <= R, fp32 sums (fused multiply-adds over the lane's slices, then the wave's DPP sum)
template <typename T, int R>
__global__ __launch_bounds__(kSkinnyThreads) void nexttoken_skinny(const T *__restrict__ x, int64_t x_stride, int n_rows, int K, int norm_in, float eps,
                                                                   const T *__restrict__ W, int V, T *__restrict__ S) {
    typedef LogitVec<T> Vec;
    extern __shared__ __attribute__((aligned(16))) unsigned char nt_smem[];
    T *xs = (T *)nt_smem;   // [R][K]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = wave; r < R; r += kSkinnyWaves) {
        if (r < n_rows) norm_round_row<T>(x + r * x_stride, K, norm_in, eps, xs + r * K);
        else
            for (int k = lane; k < K; k += 64) xs[r * K + k] = (T)0.f;
    }
    __syncthreads();
    const int kvec = K / Vec::N, groups = V / kSkinnyCls;
    for (int g = blockIdx.x * kSkinnyWaves + wave; g < groups; g += gridDim.x * kSkinnyWaves) {
        const int c0 = g * kSkinnyCls;
        float acc[kSkinnyCls][R];
#pragma unroll
        for (int c = 0; c < kSkinnyCls; ++c)
#pragma unroll
            for (int r = 0; r < R; ++r) acc[c][r] = 0.f;
#pragma unroll 2
        for (int kv = lane; kv < kvec; kv += 64) {
            Vec w[kSkinnyCls];
#pragma unroll
            for (int c = 0; c < kSkinnyCls; ++c) w[c] = ((const Vec *)(W + (int64_t)(c0 + c) * K))[kv];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const Vec xv = ((const Vec *)(xs + r * K))[kv];
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) {
                    const float xe = xv.get(e);
#pragma unroll
                    for (int c = 0; c < kSkinnyCls; ++c) acc[c][r] = __builtin_fmaf(w[c].get(e), xe, acc[c][r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float s[kSkinnyCls];
#pragma unroll
            for (int c = 0; c < kSkinnyCls; ++c) s[c] = wave_sum(acc[c][r]);
            if (lane < kSkinnyCls && r < n_rows) {
                const float v = lane == 0 ? s[0] : lane == 1 ? s[1] : lane == 2 ? s[2] : s[3];
                S[(int64_t)r * V + c0 + lane] = (T)v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the row pass
// the order-preserving integer image of a logit (no NaN reaches it)
__device__ __forceinline__ uint32_t nt_key(float l) {
    const uint32_t b = __float_as_uint(l);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float nt_exp(float l, float m, float inv_t) { return __expf((l - m) * inv_t); }
// the integer mass: ceil(e 2^44), at least 1 for a finite logit
__device__ __forceinline__ unsigned long long nt_mass(float l, float m, float inv_t) {
    if (l == -INFINITY) return 0ull;
    const unsigned long long q = __float2ull_ru(nt_exp(l, m, inv_t) * kNtMassScale);
    return q ? q : 1ull;
}
__device__ __forceinline__ unsigned long long nt_wave_sum_u64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long nt_wave_scan_u64(unsigned long long v, int lane) {   // inclusive
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// One wave: the first j in [0, n) with base + a[0] + .. + a[j] > target, and base + a[0] + .. + a[j-1]; res = {j, that sum}; j = n
// when the whole sum stays at or below target.  Lane i takes the entries [i per, (i + 1) per).
__device__ __forceinline__ void nt_find_cross(const unsigned long long *a, int n, unsigned long long base, unsigned long long target,
                                              unsigned long long *res) {
    const int lane = threadIdx.x & 63, per = (n + 63) >> 6, lo = lane * per;
    unsigned long long s = 0;
    for (int j = lo; j < lo + per && j < n; ++j) s += a[j];
    const unsigned long long incl = nt_wave_scan_u64(s, lane);
    const unsigned long long mask = __ballot(base + incl > target);
    if (mask == 0) {
        if (lane == 63) {
            res[0] = (unsigned long long)n;
            res[1] = base + incl;
        }
        return;
    }
    if (lane == __builtin_ctzll(mask)) {
        unsigned long long run = base + incl - s;
        int j = lo;
        for (; j < lo + per && j < n; ++j) {   // the lane's own entries cross, so this breaks
            if (run + a[j] > target) break;
            run += a[j];
        }
        res[0] = (unsigned long long)j;
        res[1] = run;
    }
}

struct NtRowOut {
    const float *u;
    int64_t *token;
    float *prob, *top_prob, *logits;
    int32_t *kept, *top_cls;
    uint32_t *status;
};

// NV > 0: the row's vectors stay in registers (thread t holds vectors t, t + nt, ..), NV == 0: every sweep reads the row again.
template <typename T, int NV>
__global__ __launch_bounds__(kRowThreads) void nexttoken_row(const T *__restrict__ S, int V, int64_t rows, float inv_t, int top_k, float top_p, int greedy,
                                                             int n_top, NtRowOut o) {
    typedef LogitVec<T> Vec;
    __shared__ unsigned long long hist[kNtBins];
    __shared__ unsigned long long sh_res[2], sh_acc[3];
    __shared__ float sh_v[kRowWavesMax], sh_e;
    __shared__ int sh_c[kRowWavesMax], sh_tok;
    const int64_t r = blockIdx.x;
    if (r >= rows) return;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6, nvec = V / Vec::N;
    const int steps = NV > 0 ? NV : (nvec + nt - 1) / nt;
    const Vec *row = (const Vec *)(S + r * (int64_t)V);
    Vec a[NV > 0 ? NV : 1];
    if (NV > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = tid + i * nt;
            if (idx < nvec) a[i] = row[idx];
        }
    }
    if (tid < 3) sh_acc[tid] = 0ull;
    // f(i, idx, valid, vec) for every step i, on every thread (valid: the thread has a vector in step i)
    auto sweep_vec = [&](auto &&f) {
        if (NV > 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int idx = tid + i * nt;
                // the same registers behind an opaque copy: what one sweep derives from the row (widened values, keys) would otherwise
                // be kept for the next sweep, several rows' worth of registers
                asm volatile("" : "+v"(a[i].q.x), "+v"(a[i].q.y), "+v"(a[i].q.z), "+v"(a[i].q.w));
                f(i, idx, idx < nvec, a[i]);
            }
        } else {
            for (int i = 0; i < steps; ++i) {
                const int idx = tid + i * nt;
                Vec v;
                v.q = row[idx < nvec ? idx : 0].q;
                f(i, idx, idx < nvec, v);
            }
        }
    };
    // f(cls, l) for every class of the thread, in ascending class order; -0 arrives as +0
    auto sweep = [&](auto &&f) {
        sweep_vec([&](int, int idx, bool valid, const Vec &v) {
            if (valid) {
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) f(idx * Vec::N + e, v.get(e) + 0.f);
            }
        });
    };
    // the pair (largest value, lowest class) of the workgroup from the threads' pairs; two barriers
    auto block_argmax = [&](float &v, int &c) {
        wave_argmax(v, c);
        if (lane == 0) {
            sh_v[wave] = v;
            sh_c[wave] = c;
        }
        __syncthreads();
        v = sh_v[0];
        c = sh_c[0];
        for (int w = 1; w < nw; ++w) argmax_take(v, c, sh_v[w], sh_c[w]);
        __syncthreads();
    };

    // ---- the maximum with its lowest class, the row's health, the logits output
    float m = -INFINITY;
    int m_cls = 0x7fffffff, bad = 0;
    float *lrow = o.logits ? o.logits + r * (int64_t)V : nullptr;
    sweep_vec([&](int, int idx, bool valid, const Vec &v) {
        if (!valid) return;
        float w[Vec::N];
#pragma unroll
        for (int e = 0; e < Vec::N; ++e) {
            w[e] = v.get(e);
            bad |= (w[e] != w[e]) || w[e] == INFINITY;
            if (w[e] > m) {
                m = w[e];
                m_cls = idx * Vec::N + e;
            }
        }
        if (lrow) {
#pragma unroll
            for (int e = 0; e < Vec::N; e += 4) *(float4 *)(lrow + idx * Vec::N + e) = make_float4(w[e], w[e + 1], w[e + 2], w[e + 3]);
        }
    });
    bad = __syncthreads_or(bad);
    block_argmax(m, m_cls);
    m += 0.f;
    if (bad || m == -INFINITY) {   // a NaN or +inf logit, or no finite logit at all
        if (tid == 0) {
            o.token[r] = -1;
            if (o.prob) o.prob[r] = __uint_as_float(0x7fc00000u);
            if (o.kept) o.kept[r] = 0;
            for (int j = 0; j < n_top; ++j) {
                if (o.top_cls) o.top_cls[r * n_top + j] = -1;
                if (o.top_prob) o.top_prob[r * n_top + j] = 0.f;
            }
            if (o.status) atomicOr(o.status, (uint32_t)MOT_STATUS_LOGIT_NONFINITE);
        }
        return;
    }

    // ---- radix selection: the key of the first class, in descending key order, at which base + (weights so far) exceeds target
    auto select = [&](unsigned long long target, auto &&weight) -> uint32_t {
        uint32_t prefix = 0;
        unsigned long long base = 0;
#pragma unroll 1
        for (int level = 0; level < 3; ++level) {
            const int shift = level == 0 ? 21 : level == 1 ? 10 : 0, up = level == 1 ? 21 : 10, nb = level < 2 ? 2048 : 1024;
            for (int b = tid; b < nb; b += nt) hist[b] = 0ull;
            __syncthreads();
            sweep([&](int, float l) {
                const uint32_t key = nt_key(l);
                if (level == 0 || (key >> up) == prefix) {
                    const unsigned long long w = weight(key, l);
                    if (w) atomicAdd(&hist[nb - 1 - (int)((key >> shift) & (uint32_t)(nb - 1))], w);
                }
            });
            __syncthreads();
            if (wave == 0) nt_find_cross(hist, nb, base, target, sh_res);
            __syncthreads();
            const int j = (int)sh_res[0];   // below nb: both callers' targets lie below the sum of all weights; clamped all the same
            base = sh_res[1];
            prefix = (prefix << (level < 2 ? 11 : 10)) | (uint32_t)(nb - 1 - (j < nb ? j : nb - 1));
        }
        return prefix;
    };

    // ---- top-k: the k-th largest key; ties with it stay
    uint32_t cut = 0;   // the classes with key >= cut survive
    if (top_k > 0 && top_k < V) cut = select((unsigned long long)(top_k - 1), [](uint32_t, float) { return 1ull; });
    // ---- top-p over the survivors: a class stays when the mass of the strictly larger logits is <= top_p Z1; a tie group stays whole
    if (top_p < 1.f) {
        unsigned long long z1 = 0;
        sweep([&](int, float l) { z1 += nt_key(l) >= cut ? nt_mass(l, m, inv_t) : 0ull; });
        z1 = nt_wave_sum_u64(z1);
        if (lane == 0) atomicAdd(&sh_acc[0], z1);
        __syncthreads();
        z1 = sh_acc[0];
        const unsigned long long thr = (unsigned long long)((double)top_p * (double)z1);
        const uint32_t kcut = cut;
        cut = select(thr, [&](uint32_t key, float l) { return key >= kcut ? nt_mass(l, m, inv_t) : 0ull; });
        if (cut < kcut) cut = kcut;
    }
    // ---- the kept count and their mass Z
    unsigned long long cnt = 0, z = 0;
    sweep([&](int, float l) {
        if (nt_key(l) >= cut) {
            ++cnt;
            z += nt_mass(l, m, inv_t);
        }
    });
    cnt = nt_wave_sum_u64(cnt);
    z = nt_wave_sum_u64(z);
    if (lane == 0) {
        atomicAdd(&sh_acc[1], cnt);
        atomicAdd(&sh_acc[2], z);
    }
    __syncthreads();
    cnt = sh_acc[1];
    z = sh_acc[2];
    const double zf = (double)z * kNtMassUnit;

    // ---- the result
    if (greedy) {
        if (tid == 0) {
            sh_tok = m_cls;
            sh_e = 1.f;
        }
    } else {
        float uu = o.u[r];
        uu = uu >= 0.f ? uu : 0.f;   // a NaN counts as 0
        uu = fminf(uu, 0.99999994f);
        const unsigned long long tq = (unsigned long long)((double)uu * (double)z);
        // the kept mass of the spans (step i, wave w), in class order
        sweep_vec([&](int i, int idx, bool valid, const Vec &v) {
            unsigned long long s = 0;
            if (valid) {
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) {
                    const float l = v.get(e) + 0.f;
                    s += nt_key(l) >= cut ? nt_mass(l, m, inv_t) : 0ull;
                }
            }
            s = nt_wave_sum_u64(s);
            if (lane == 0) hist[i * nw + wave] = s;
        });
        __syncthreads();
        if (wave == 0) nt_find_cross(hist, steps * nw, 0ull, tq, sh_res);
        __syncthreads();
        const int span = (int)sh_res[0];
        const unsigned long long before = sh_res[1];
        if (span >= steps * nw) {   // rounding let no class exceed u Z: the last kept class
            float none = -INFINITY;
            int last = -1;
            float last_e = 0.f;
            sweep([&](int cls, float l) {
                if (nt_key(l) >= cut) {
                    last = cls;
                    last_e = nt_exp(l, m, inv_t);
                }
            });
            // the largest class: argmax over (class as a value); classes are below 2^24, exact in fp32
            float lv = last >= 0 ? (float)last : none;
            int li = last >= 0 ? __float_as_int(last_e) : 0;
            // equal values cannot come from two threads, so the tie rule of argmax_take never decides
            block_argmax(lv, li);
            if (tid == 0) {
                sh_tok = (int)lv;
                sh_e = __int_as_float(li);
            }
        } else {
            const int si = span / nw, sw = span - si * nw;
            sweep_vec([&](int i, int idx, bool valid, const Vec &v) {
                if (i != si || wave != sw) return;   // wave-uniform
                unsigned long long q[Vec::N], s = 0;
#pragma unroll
                for (int e = 0; e < Vec::N; ++e) {
                    const float l = v.get(e) + 0.f;
                    q[e] = valid && nt_key(l) >= cut ? nt_mass(l, m, inv_t) : 0ull;
                    s += q[e];
                }
                const unsigned long long incl = nt_wave_scan_u64(s, lane);
                const unsigned long long mask = __ballot(before + incl > tq);
                if (mask && lane == __builtin_ctzll(mask)) {
                    unsigned long long run = before + incl - s;
                    int pick = 0;
                    bool found = false;
#pragma unroll
                    for (int e = 0; e < Vec::N; ++e) {
                        if (!found && q[e] && run + q[e] > tq) {
                            pick = e;
                            found = true;
                        }
                        run += found ? 0ull : q[e];
                    }
                    sh_tok = idx * Vec::N + pick;
                    sh_e = nt_exp(v.get(pick) + 0.f, m, inv_t);
                }
            });
        }
    }
    __syncthreads();
    if (tid == 0) {
        o.token[r] = sh_tok;
        if (o.prob) o.prob[r] = (float)((double)sh_e / zf);
        if (o.kept) o.kept[r] = (int32_t)cnt;
    }
    // ---- the n_top largest filtered probabilities: n_top rounds of the workgroup's argmax over what lies behind the last pair
    float pl = INFINITY;
    int pc = -1;
    for (int j = 0; j < n_top; ++j) {
        float bv = -INFINITY;
        int bc = 0x7fffffff;
        sweep([&](int cls, float l) {
            if (nt_key(l) >= cut && (l < pl || (l == pl && cls > pc)) && (l > bv || bc == 0x7fffffff)) {
                bv = l;
                bc = cls;
            }
        });
        block_argmax(bv, bc);
        if (tid == 0) {
            const bool any = bc != 0x7fffffff;
            if (o.top_cls) o.top_cls[r * n_top + j] = any ? bc : -1;
            if (o.top_prob) o.top_prob[r * n_top + j] = any ? (float)((double)nt_exp(bv, m, inv_t) / zf) : 0.f;
        }
        pl = bv;
        pc = bc;   // nothing left: bc stays at its sentinel, so no class lies behind the pair in the later rounds
    }
}

// ---------------------------------------------------------------------------------------------- the call
struct NtGeom {
    int64_t rows, chunk, x_stride;
    int K, V, norm_in;
    bool bf16;
    float eps;
};

struct NtWs {   // carve of the workspace, offsets in bytes
    size_t S, hg, total;
};

NtWs nt_ws(const NtGeom &g) {
    const size_t e = g.bf16 ? 2 : 4;
    Arena a;
    NtWs w{};
    w.S = a.take((size_t)g.chunk * g.V * e);
    w.hg = a.take(g.rows > kSkinnyRows ? (size_t)g.chunk * g.K * e : 0);
    w.total = a.o;
    return w;
}

// every refusal of the call but the workspace's, before any HIP call; `fn` starts the messages
int nt_check(const MotNextTokenDesc *d, NtGeom *out, const char *fn) {
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotNextTokenDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotNextTokenDesc));
    if (int rc = wide_shape_check(fn, d->dtype, d->n_rows, d->model_dim, d->vocab)) return rc;
    const int e = d->dtype == MOT_BF16 ? 2 : 4;
    if (d->x_stride < d->model_dim) return set_error(MOT_ESHAPE, "%s: x_stride %lld below model_dim %d", fn, (long long)d->x_stride, d->model_dim);
    if ((d->x_stride * e) & 15)
        return set_error(MOT_EUNSUPPORTED, "%s: x_stride %lld must keep the rows of x 16-byte aligned", fn, (long long)d->x_stride);
    if (!(d->temperature > 0.f) || d->temperature > 3.4028234e38f)
        return set_error(MOT_EINVAL, "%s: temperature %g must be positive and finite", fn, (double)d->temperature);
    if (d->top_k < 0) return set_error(MOT_EINVAL, "%s: top_k %d must not be negative (0: no cut)", fn, d->top_k);
    if (!(d->top_p > 0.f)) return set_error(MOT_EINVAL, "%s: top_p %g must be positive (>= 1: no cut)", fn, (double)d->top_p);
    if (d->n_top < 0 || d->n_top > kNtMaxTop) return set_error(MOT_EINVAL, "%s: n_top %d must lie in 0..%d", fn, d->n_top, kNtMaxTop);
    if (d->reserved) return set_error(MOT_EINVAL, "%s: reserved %d must be 0", fn, d->reserved);
    if (!d->x || !d->weight || !d->token) return set_error(MOT_EINVAL, "%s: null x / weight / token", fn);
    if (!d->greedy && !d->u) return set_error(MOT_EINVAL, "%s: null u without greedy (the draw is the caller's)", fn);
    if (((uintptr_t)d->x & 15) || ((uintptr_t)d->weight & 15) || ((uintptr_t)d->logits & 15))
        return set_error(MOT_EUNSUPPORTED, "%s: x, weight and logits must be 16-byte aligned", fn);
    NtGeom &g = *out;
    g.rows = d->n_rows;
    g.x_stride = d->x_stride;
    g.K = d->model_dim;
    g.V = d->vocab;
    g.norm_in = d->norm_in ? 1 : 0;
    g.bf16 = d->dtype == MOT_BF16;
    g.eps = d->eps > 0.f ? d->eps : kHeadEps;
    g.chunk = head_chunk_rows(kChunkBytes, ((int64_t)g.V + g.K) * e, g.rows);   // the heads' rule: a chunk's logits stay below kChunkBytes
    return MOT_OK;
}

template <typename T, int R>
int launch_skinny(const T *x, const NtGeom &g, int n, const T *W, T *S, hipStream_t stream) {
    static std::atomic<uint64_t> lds_ok{0};
    const size_t lds = (size_t)R * g.K * sizeof(T);
    if (lds > (48u << 10))
        if (int rc = ensure_max_dyn_lds((const void *)nexttoken_skinny<T, R>, lds_ok, "nexttoken_skinny")) return rc;
    const int need = (g.V / kSkinnyCls + kSkinnyWaves - 1) / kSkinnyWaves;
    hipLaunchKernelGGL((nexttoken_skinny<T, R>), dim3((unsigned)(need < kSkinnyGrid ? need : kSkinnyGrid)), dim3(kSkinnyThreads), lds, stream, x, g.x_stride,
                       n, g.K, g.norm_in, g.eps, W, g.V, S);
    return check_launch("nexttoken_skinny");
}

template <typename T>
int launch_nt_row(const T *S, const NtGeom &g, const MotNextTokenDesc &d, int64_t n, const NtRowOut &o, hipStream_t stream) {
    int nt, nv;
    rows_geometry<T>(g.V, nt, nv);
    const float inv_t = 1.f / d.temperature;
#define MOT_NEXTTOKEN_ROW(NV) \
    hipLaunchKernelGGL((nexttoken_row<T, NV>), dim3((unsigned)n), dim3(nt), 0, stream, S, g.V, n, inv_t, d.top_k, d.top_p, d.greedy ? 1 : 0, d.n_top, o)
    // eight 16-byte vectors a thread stay in registers: 32 768 classes in fp32, 65 536 in bf16.  With sixteen (fp32 up to 65 536) the
    // compiler spills 224 bytes a lane under the 128 registers of a 1024-thread workgroup, so those rows are read again from L2.
    if (nv <= 4) MOT_NEXTTOKEN_ROW(4);
    else if (nv <= 8) MOT_NEXTTOKEN_ROW(8);
    else MOT_NEXTTOKEN_ROW(0);
#undef MOT_NEXTTOKEN_ROW
    return check_launch("nexttoken_row");
}

template <typename T>
int nt_run(const MotNextTokenDesc &d, const NtGeom &g, const NtWs &w, hipStream_t stream) {
    constexpr bool BF = sizeof(T) == 2;
    unsigned char *ws = (unsigned char *)d.workspace;
    T *S = (T *)(ws + w.S), *hg = (T *)(ws + w.hg);
    const T *X = (const T *)d.x, *W = (const T *)d.weight;
    for (int64_t r0 = 0; r0 < g.rows; r0 += g.chunk) {
        const int64_t n = g.rows - r0 < g.chunk ? g.rows - r0 : g.chunk;
        const T *x = X + r0 * g.x_stride;
        int rc;
        if (g.rows <= kSkinnyRows) {   // one chunk
            const int k = (int)n;
            rc = k <= 1 ? launch_skinny<T, 1>(x, g, k, W, S, stream)
               : k <= 2 ? launch_skinny<T, 2>(x, g, k, W, S, stream)
               : k <= 4 ? launch_skinny<T, 4>(x, g, k, W, S, stream)
               : k <= 8 ? launch_skinny<T, 8>(x, g, k, W, S, stream)
                        : launch_skinny<T, 16>(x, g, k, W, S, stream);
            if (rc) return rc;
        } else {
            hipLaunchKernelGGL(nexttoken_rows_in<T>, dim3((unsigned)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, x, g.x_stride, n, g.K, g.norm_in,
                               g.eps, hg);
            if ((rc = check_launch("nexttoken_rows_in"))) return rc;
            if ((rc = launch_product_nt(head_dtype<T>, hg, g.K, n, W, g.K, g.K, g.V, S, g.V, BF, nullptr, false, stream))) return rc;
        }
        NtRowOut o{};
        o.u = d.u ? d.u + r0 : nullptr;
        o.token = d.token + r0;
        o.prob = d.prob ? d.prob + r0 : nullptr;
        o.kept = d.kept ? d.kept + r0 : nullptr;
        o.top_cls = d.top_cls ? d.top_cls + r0 * d.n_top : nullptr;
        o.top_prob = d.top_prob ? d.top_prob + r0 * d.n_top : nullptr;
        o.logits = d.logits ? d.logits + r0 * g.V : nullptr;
        o.status = d.status;
        if ((rc = launch_nt_row<T>(S, g, d, n, o, stream))) return rc;
    }
    return MOT_OK;
}

}  // namespace

size_t next_token_workspace_bytes(const MotNextTokenDesc *d) {
    NtGeom g;
    if (nt_check(d, &g, "mot_next_token_workspace_bytes") || g.rows == 0) return 0;
    return nt_ws(g).total;
}

int launch_next_token(const MotNextTokenDesc *d, hipStream_t stream) {
    static const char fn[] = "mot_next_token";
    NtGeom g;
    if (int rc = nt_check(d, &g, fn)) return rc;
    if (g.rows == 0) return MOT_OK;
    const NtWs w = nt_ws(g);
    if (!d->workspace || d->workspace_bytes < w.total)
        return set_error(MOT_EWORKSPACE, "%s: workspace %zu bytes < %zu", fn, d->workspace ? d->workspace_bytes : (size_t)0, w.total);
    if ((uintptr_t)d->workspace & 15) return set_error(MOT_EUNSUPPORTED, "%s: workspace must be 16-byte aligned", fn);
    return g.bf16 ? nt_run<__bf16>(*d, g, w, stream) : nt_run<float>(*d, g, w, stream);
}

}  // namespace mot
