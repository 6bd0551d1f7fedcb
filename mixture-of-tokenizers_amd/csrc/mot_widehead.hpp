// mot_widehead.hpp -- the host side of the V-wide cross-entropy heads (mot_tokhead.hip: the token-level head, mot_plainhead.hip: the
// plain head and its compacted form), written once: the shape check (mot_nexttoken.hip takes it too), the geometry with the chunk
// rule, the workspace carve, the pointer checks with the dtype dispatch, and the chunk loop.  A head supplies its descriptor's own
// checks and the arithmetic of the row pass (the Stat of wide_rows, mot_headrows.hpp), which also tells the loop whether the loss
// divides by the constant n_rows or by the device count of kept rows.
#pragma once
#include "mot_headrows.hpp"

namespace mot {

static inline bool head_dtype_ok(int dtype) { return dtype == MOT_F32 || dtype == MOT_BF16; }

// the shape refusals every V-wide call shares, before any HIP call; `fn` starts the messages.  chunk_rows: null for a call without
// that field
static inline int wide_shape_check(const char *fn, int dtype, int64_t n_rows, int model_dim, int vocab, const int32_t *chunk_rows = nullptr) {
    if (!head_dtype_ok(dtype)) return set_error(MOT_EUNSUPPORTED, "%s: dtype %d is not built", fn, dtype);
    if (n_rows < 0 || n_rows > 0x7fffffffLL || model_dim <= 0 || vocab <= 0)
        return set_error(MOT_ESHAPE, "%s: n_rows %lld, model_dim %d, vocab %d", fn, (long long)n_rows, model_dim, vocab);
    if (vocab % kMinV || vocab > kMaxV)
        return set_error(MOT_EUNSUPPORTED, "%s: vocab %d must be a multiple of %d and at most %d", fn, vocab, kMinV, kMaxV);
    if (model_dim % 16 || model_dim > kMaxD)
        return set_error(MOT_EUNSUPPORTED, "%s: model_dim %d must be a multiple of 16 and at most %d", fn, model_dim, kMaxD);
    if (!chunk_rows) return MOT_OK;
    if (*chunk_rows < 0 || *chunk_rows % 32)
        return set_error(MOT_ESHAPE, "%s: chunk_rows %d must be 0 (the library's choice) or a multiple of 32", fn, *chunk_rows);
    if ((int64_t)*chunk_rows * vocab > 0x7fffffffLL)
        return set_error(MOT_EUNSUPPORTED, "%s: chunk_rows %d x vocab %d exceeds 2^31 logits a chunk", fn, *chunk_rows, vocab);
    return MOT_OK;
}

struct WideGeom {
    int64_t rows = 0, over = 0, chunk = 0, ignore = -1;   // over: the rows the chunks run over: n_rows, or cap of the compacted form
    int K = 0, V = 0, norm_in = 0, group = 0;
    bool bf16 = false, grad_x = false, counted = false, compact = false;   // counted: the divisor is the device count of kept rows
    float eps = kHeadEps;
};

// The fields MotTokenHeadDesc and MotPlainHeadDesc share, of a descriptor that passed its checks, and the chunk rule over `over`
// rows: n_rows, or the compacted form's cap.  This is the one place the rule is applied.
template <typename Desc>
void wide_geom_fill(const Desc &d, int64_t over, WideGeom &g) {
    g.rows = d.n_rows;
    g.over = over;
    g.K = d.model_dim;
    g.V = d.vocab;
    g.norm_in = d.norm_in ? 1 : 0;
    g.bf16 = d.dtype == MOT_BF16;
    g.grad_x = d.dx != nullptr;
    g.eps = d.eps > 0.f ? d.eps : kHeadEps;
    if (d.chunk_rows)
        g.chunk = over < d.chunk_rows ? over : d.chunk_rows;
    else   // the library's choice: a chunk's logits and u stay below kChunkBytes
        g.chunk = head_chunk_rows(kChunkBytes, (int64_t)g.V * (g.bf16 ? 2 : 4) + (int64_t)g.K * 4, over);
}

struct WideWs {   // carve of the workspace, offsets in bytes (Arena: every piece starts on 256 bytes); a piece the call does not use takes none
    size_t term, part, kept, scan, idx, tg, hg, S, u, WT, ev_loss, ev_pred, ev_rank, total;
};

static inline WideWs wide_ws(const WideGeom &g) {
    const size_t e = g.bf16 ? 2 : 4, slots = g.compact ? (size_t)g.over * 4 : 0, cchunk = g.compact ? (size_t)g.chunk : 0;
    Arena a;
    WideWs w{};
    w.term = a.take((size_t)g.over * 4);
    w.part = a.take((size_t)kLossParts * 8);
    w.kept = a.take(g.counted ? 8 : 0);
    w.scan = a.take(g.compact ? (size_t)kLossParts * 8 : 0);
    w.idx = a.take(slots);
    w.tg = a.take(cchunk * 8);
    w.hg = a.take(cchunk * g.K * e);
    w.S = a.take((size_t)g.chunk * g.V * e);
    w.u = a.take(g.grad_x ? (size_t)g.chunk * g.K * 4 : 0);
    w.WT = a.take(g.grad_x && g.bf16 ? (size_t)g.V * g.K * 2 : 0);
    w.ev_loss = a.take(slots);   // the compacted evaluation's per-slot rows; 12 bytes a slot, carved for both calls so that one query serves them
    w.ev_pred = a.take(slots);
    w.ev_rank = a.take(slots);
    w.total = a.o;
    return w;
}

// The compaction context of the chunk loop (mot_plain_head_compact_*): the kept rows' numbers idx[0, kept) behind the scan's
// scratch, the chunk's gathered rows hg (in the call's dtype) with their targets tg, and the evaluation's per-slot rows.  Only a
// counted Stat can be compacted; it supplies the launchers compact_index / _zero_dropped / _gather<T> / _chain_scatter<T> /
// _eval_rows as static members (PlainStat, mot_plainhead.hip), each of which also takes the device count `kept`.
struct WideCompact {
    int32_t *idx;
    long long *scan;
    void *hg;
    int64_t *tg;
    HeadEvalRows slot;
};

// The chunk loop.  A chunk's logits s = x W^T are one product on the shared launchers into the chunk scratch S (fp32, or bf16 in
// bf16 mode: the reference's own rounding point), wide_rows forms the loss terms and writes G over the logits, u = G W and
// dW += G^T x are two more products, and the heads' wave-per-row chain closes dx: a chunk's logits are formed once and a training
// step costs three products.  `ev` set: the evaluation call (no gradients): the row pass also writes ev's rows, and the counts are
// closed behind the loss.  The compacted form gathers the chunk's rows in front and scatters the chain behind.
template <typename T, typename Stat, typename Desc>
int wide_run(const Desc &d, const WideGeom &g, const WideWs &w, const MotHeadEvalOut *ev, hipStream_t stream) {
    constexpr bool BF = sizeof(T) == 2;
    unsigned char *ws = (unsigned char *)d.workspace;
    float *term = (float *)(ws + w.term), *u = (float *)(ws + w.u);
    long long *kept = (long long *)(ws + w.kept);
    T *S = (T *)(ws + w.S), *WT = (T *)(ws + w.WT);
    const T *X = (const T *)d.x, *W = (const T *)d.weight;
    const bool grad = d.dx || d.dW;
    const WideCompact slots{(int32_t *)(ws + w.idx), (long long *)(ws + w.scan), ws + w.hg, (int64_t *)(ws + w.tg),
                            {(float *)(ws + w.ev_loss), (int32_t *)(ws + w.ev_pred), (int32_t *)(ws + w.ev_rank)}};
    constexpr bool CX = Stat::kCounted;   // the compaction's branches exist in a counted head's loop alone
    const WideCompact *cx = CX && g.compact ? &slots : nullptr;
    const HeadEvalRows ev_out = ev ? HeadEvalRows{ev->row_loss, ev->pred, ev->rank} : HeadEvalRows{};
    const HeadEvalRows ev_rows = cx && ev ? cx->slot : ev_out;
    const int norm_rows = cx ? 0 : g.norm_in;             // the gather has normed the compacted rows
    uint32_t *row_status = cx ? nullptr : d.status;       // and the index pass has reported their targets
    int rc = MOT_OK;
    if constexpr (CX) {
        if (cx) rc = Stat::compact_index(d.targets, g, *cx, kept, d.status, stream);
        else rc = launch_head_kept(d.targets, g.rows, g.V, g.ignore, ws + w.part, kept, stream);   // the row pass divides by it
        if (rc) return rc;
    }
    if (d.dW && (rc = launch_zero_words(d.dW, (int64_t)g.V * g.K, stream))) return rc;
    if constexpr (CX)
        if (cx && d.dx && (rc = Stat::compact_zero_dropped(d.targets, g, kept, d.dx, stream))) return rc;
    if (BF && d.dx && (rc = launch_transpose_bf16(W, g.V, g.K, WT, stream))) return rc;   // WT[k][v]: the operand of u = G W on the bf16 launcher
    for (int64_t r0 = 0; r0 < g.over; r0 += g.chunk) {
        const int64_t n = g.over - r0 < g.chunk ? g.over - r0 : g.chunk;
        const T *x = cx ? (const T *)cx->hg : X + r0 * g.K;
        const int64_t *tgt = cx ? cx->tg : d.targets + r0;
        if constexpr (CX)
            if (cx && (rc = Stat::template compact_gather<T>(X, d.targets, g, *cx, kept, r0, n, stream))) return rc;
        if ((rc = launch_product_nt(head_dtype<T>, x, g.K, n, W, g.K, g.K, g.V, S, g.V, BF, nullptr, false, stream))) return rc;   // s = x W^T for the chunk's rows, in T
        const typename Stat::Args sa = Stat::args(d, g, kept, r0);
        if (ev)
            rc = launch_wide_rows<T, Stat, false, true>(S, g.V, x, g.K, norm_rows, g.eps, tgt, n, sa, term + r0, row_status, ev_rows.at(r0), stream);
        else if (grad)
            rc = launch_wide_rows<T, Stat, true, false>(S, g.V, x, g.K, norm_rows, g.eps, tgt, n, sa, term + r0, row_status, {}, stream);
        else
            rc = launch_wide_rows<T, Stat, false, false>(S, g.V, x, g.K, norm_rows, g.eps, tgt, n, sa, term + r0, row_status, {}, stream);
        if (rc) return rc;
        if (d.dx) {   // u = G W, then the row chain of the plain norm (L = 0), of each valid slot straight into its row of dx when compacted
            if ((rc = launch_product_nn(head_dtype<T>, S, g.V, n, BF ? WT : W, BF ? g.V : g.K, g.V, g.K, u, g.K, stream))) return rc;
            if constexpr (CX)
                if (cx && (rc = Stat::template compact_chain_scatter<T>(X, u, g, *cx, kept, r0, n, (T *)d.dx, stream))) return rc;
            if (!cx && (rc = launch_head_chain<T>(x, u, g.K, n, 0, g.norm_in, g.eps, (T *)d.dx + r0 * g.K, stream))) return rc;
        }
        if (d.dW && (rc = launch_product_tn(head_dtype<T>, S, g.V, g.V, x, g.K, g.K, n, d.dW, g.K, stream))) return rc;   // dW += G^T x
    }
    double *part = (double *)(ws + w.part);
    if (Stat::kCounted) rc = launch_head_loss_kept(term, g.over, part, kept, d.loss, stream);
    else rc = launch_head_loss(term, g.rows, part, 1.0 / (double)g.rows, d.loss, stream);
    if (rc || !ev) return rc;
    if constexpr (CX)
        if (cx && (ev->row_loss || ev->pred || ev->rank) && (rc = Stat::compact_eval_rows(d.targets, g, *cx, kept, ev_out, stream))) return rc;
    if (ev->counts) {   // per row, or per group of group_rows rows; a counted head leaves the dropped rows out of their groups
        const int per = g.group > 0 ? g.group : 1;
        return launch_head_eval_counts(ev->pred, d.targets, g.rows / per, per, g.V, part, ev->counts, g.group > 0 ? 3 : 2, stream, Stat::kCounted ? 1 : 0,
                                       g.ignore);
    }
    return MOT_OK;
}

// the checks behind the descriptor's own, then the launches in the descriptor's dtype; `fn` starts the messages
template <typename Stat, typename Desc>
int wide_launch(const Desc &d, const WideGeom &g, const MotHeadEvalOut *ev, const char *fn, hipStream_t stream) {
    if (!d.x || !d.weight || !d.targets || !d.loss) return set_error(MOT_EINVAL, "%s: null x / weight / targets / loss", fn);
    if (g.rows == 0) return set_error(MOT_ESHAPE, "%s: no rows (the mean over zero targets is undefined)", fn);
    const WideWs w = wide_ws(g);
    if (!d.workspace || d.workspace_bytes < w.total)
        return set_error(MOT_EWORKSPACE, "%s: workspace %zu bytes < %zu", fn, d.workspace ? d.workspace_bytes : (size_t)0, w.total);
    if (((uintptr_t)d.x & 15) || ((uintptr_t)d.weight & 15) || ((uintptr_t)d.workspace & 15) || ((uintptr_t)d.dx & 15) || ((uintptr_t)d.dW & 15))
        return set_error(MOT_EUNSUPPORTED, "%s: x, weight, workspace, dx and dW must be 16-byte aligned", fn);
    return g.bf16 ? wide_run<__bf16, Stat>(d, g, w, ev, stream) : wide_run<float, Stat>(d, g, w, ev, stream);
}

}  // namespace mot
