// mot_tokhead.hip -- the token-level output head, the last five lines of every training script of the reference:
//   scaled-pre-train/train_gpt.py:619-623 (byte_mixout_method "noop"):  x = norm(x); l = lm_head(x); z = 30 sigmoid(l.float() / 7.5); CE(z, y)
//   modded-nanogpt/runs/71_*.py:331-334 (all 50 runs):                 x = norm(x); l = x W^T;       z = 15 l rsqrt(l^2 + 225);   CE(z, y)
// over a vocabulary of 50 304 rows, forward and backward in ONE call and without any N x V tensor.
//
// Per row r of x [N, D], W [V, D], y [N]:  c_r = (mean(x_r^2) + eps)^-1/2 (1 without norm_in),  l = c_r (x_r W^T),  z = cap(l).
// z is bounded (0 < z < 30, |z| < 15), so lse = zmax + log sum exp(z - zmax) with the constant zmax: no max pass.
//   loss    = (1 / N) sum_r (lse_r - z_r[y_r])                       fixed-order double sum (mot_headcore.hip)
//   dL/dl_r = (1 / N) (softmax(z_r) - onehot(y_r)) dz/dl,   G_r = c_r dL/dl_r,   u = G W,   dW = G^T x,
//   dx_r    = u_r - c_r^2 (x_r . u_r / D) x_r  (norm_in),  u_r (else)
// A target outside [0, V) addresses nothing: its term leaves the sum (the mean still divides by N), its row of G is zero, so its row
// of dx is exactly zero and it adds nothing to dW; MOT_STATUS_TARGET_OOR is raised.
//
// The rows run in chunks on the V-wide heads' one chunk loop (wide_run, mot_widehead.hpp): three products a training step, the logits
// of a chunk formed once in the chunk scratch (fp32, or bf16 in bf16 mode: the reference's own rounding point, CastedLinear returns
// bf16).  The gradients are those of grad_loss = 1; the caller scales them.  mot_token_head_eval is the loss call without gradients
// whose row pass also writes every row's loss term, the class of its largest stored logit and the number of stored logits above the
// target's (include/mot.h).
// This unit holds TokStat, the softcapped arithmetic of the shared row pass wide_rows (mot_headrows.hpp), and the descriptor's
// checks; the shape check, the geometry, the carve and the loop are mot_widehead.hpp's, row_scale, the products, the chain and the
// loss's sum the heads' shared ones (mot_headcore.hpp).
#include "mot_widehead.hpp"

namespace mot {
namespace {

// z = cap(l) and dz/dl
template <int CAP>
__device__ __forceinline__ float softcap(float l, float &dz) {
    if (CAP == MOT_SOFTCAP_SIGMOID30) {
        const float s = 1.f / (1.f + __expf(-l * (1.f / 7.5f)));
        dz = 4.f * s * (1.f - s);
        return 30.f * s;
    } else {
        const float r = rsqrtf(l * l + 225.f);
        dz = 3375.f * r * r * r;
        return 15.f * l * r;
    }
}
template <int CAP>
__device__ __forceinline__ float softcap_max() { return CAP == MOT_SOFTCAP_SIGMOID30 ? 30.f : 15.f; }

// sum exp(z - zmax) over one vector, and z[y] when the vector holds class y (ey: its element there, else -1)
template <typename T, int CAP>
__device__ __forceinline__ float vec_stats(const LogitVec<T> &a, float c, int ey, float &zy) {
    float se = 0.f;
#pragma unroll
    for (int e = 0; e < LogitVec<T>::N; ++e) {
        float dz;
        const float z = softcap<CAP>(c * a.get(e), dz);
        se += __expf(z - softcap_max<CAP>());
        if (e == ey) zy = z;
    }
    return se;
}

// The softcapped head's share of wide_rows.  z is bounded, so the statistics are a single sweep against the constant maximum; every
// in-range row is kept and the mean divides by the constant n_rows.
template <int CAP>
struct TokStat {
    static constexpr bool kCounted = false;
    struct Args {
        float inv_n;
        float *row_stats;   // optional: lse of the chunk's rows, and stats_stride further on their factors c
        int64_t stats_stride;
    };
    struct alignas(16) Lds {
        float se[kRowWavesMax], zy[kRowWavesMax];
    };
    float se, zy, lse, scale;

    static Args args(const MotTokenHeadDesc &d, const WideGeom &g, const long long *, int64_t r0) {
        return {(float)(1.0 / (double)g.rows), d.row_stats ? d.row_stats + r0 : nullptr, g.rows};
    }
    static __device__ __forceinline__ bool keeps(bool in_range, int64_t, const Args &) { return in_range; }
    static __device__ __forceinline__ bool oor(bool in_range, int64_t, const Args &) { return !in_range; }
    template <typename T, int NV, typename E>
    __device__ __forceinline__ void sweep(const RowVecs<T, NV> &rv, float c, int yvec, int yel, Lds &, E eval) {
        se = zy = 0.f;
        rv.each([&](int idx, const LogitVec<T> &v) __attribute__((always_inline)) {
            se += vec_stats<T, CAP>(v, c, idx == yvec ? yel : -1, zy);
            eval(idx, v);
        });
    }
    __device__ __forceinline__ float close(Lds &sh) {
        se = rows_block_sum(se, sh.se);
        zy = rows_block_sum(zy, sh.zy);   // one thread holds z[y], the others 0
        lse = softcap_max<CAP>() + __logf(se);
        return lse - zy;
    }
    __device__ __forceinline__ void store_stats(const Args &a, int64_t r, float c) const {
        if (a.row_stats) {
            a.row_stats[r] = lse;
            a.row_stats[a.stats_stride + r] = c;
        }
    }
    // G = c (1 / N) dz/dl (exp(z - lse) - onehot); scale = c / N, or 0 for a dropped row
    __device__ __forceinline__ void grad_prep(bool keep, float c, const Args &a) { scale = keep ? c * a.inv_n : 0.f; }
    __device__ __forceinline__ float grad(float s, float c, bool hit) const {
        float dz;
        const float z = softcap<CAP>(c * s, dz);
        const float p = __expf(z - lse);
        return scale * dz * (p - (hit ? 1.f : 0.f));
    }
};

}  // namespace

static int token_head_geom(const MotTokenHeadDesc *d, WideGeom *g, const char *fn = "token_head") {
    if (!d) return set_error(MOT_EINVAL, "%s: null descriptor", fn);
    if (d->struct_size != sizeof(MotTokenHeadDesc))
        return set_error(MOT_EINVAL, "%s: struct_size %u != %zu (ABI mismatch)", fn, d->struct_size, sizeof(MotTokenHeadDesc));
    if (head_dtype_ok(d->dtype) && d->softcap != MOT_SOFTCAP_SIGMOID30 && d->softcap != MOT_SOFTCAP_RSQRT15)   // behind the dtype's refusal
        return set_error(MOT_EUNSUPPORTED, "%s: softcap %d is not built (sigmoid30 and rsqrt15 are)", fn, d->softcap);
    if (int rc = wide_shape_check(fn, d->dtype, d->n_rows, d->model_dim, d->vocab, &d->chunk_rows)) return rc;
    wide_geom_fill(*d, d->n_rows, *g);
    return MOT_OK;
}

int token_head_check(const MotTokenHeadDesc *d) {
    WideGeom g;
    return token_head_geom(d, &g);
}

size_t token_head_workspace_bytes(const MotTokenHeadDesc &d) {
    WideGeom g;
    if (token_head_geom(&d, &g) || g.rows == 0) return 0;
    return wide_ws(g).total;
}

static int token_head_launch(const MotTokenHeadDesc &d, const WideGeom &g, const MotHeadEvalOut *ev, const char *fn, hipStream_t stream) {
    return d.softcap == MOT_SOFTCAP_SIGMOID30 ? wide_launch<TokStat<MOT_SOFTCAP_SIGMOID30>>(d, g, ev, fn, stream)
                                              : wide_launch<TokStat<MOT_SOFTCAP_RSQRT15>>(d, g, ev, fn, stream);
}

int launch_token_head_fwd(const MotTokenHeadDesc &d, hipStream_t stream) {
    WideGeom g;
    int rc = token_head_geom(&d, &g);
    if (rc) return rc;
    return token_head_launch(d, g, nullptr, "token_head", stream);
}

int launch_token_head_eval(const MotTokenHeadDesc *d, const MotHeadEvalOut *out, hipStream_t stream) {
    static const char fn[] = "mot_token_head_eval";
    WideGeom g;
    int rc = token_head_geom(d, &g, fn);
    if (rc || (rc = head_eval_check(fn, out))) return rc;
    if (d->dx || d->dW) return set_error(MOT_EINVAL, "%s: dx / dW set: the evaluation forms no gradients (mot_token_head_fwd does)", fn);
    return token_head_launch(*d, g, out, fn, stream);
}

}  // namespace mot
