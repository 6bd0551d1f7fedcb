// mot_desc.hpp -- host-side pieces that the descriptor front-ends share (mot_bytefc.hip, mot_bytecat.hip, mot_values.hip,
// mot_valuemix.hip, mot_splitx0.hip): the workspace arena, the view of a descriptor's byte-id source with its checks, the
// workspace check, and the byte ids from the token->byte table.  No device code.  A new front-end uses these.
// The output heads carve their workspaces with the arena too (mot_headcore.hpp).
#pragma once
#include "mot_internal.hpp"
#include "mot_tile.hpp"   // kPull*

namespace mot {

inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Workspace layouts: take() hands out the offset of the next piece, rounded up to `align` (bytes by default; a layout in floats counts floats).
struct Arena {
    size_t o = 0, align = 256;
    size_t take(size_t n) { const size_t at = o; o += (n + align - 1) & ~(align - 1); return at; }
};

// Where a call's byte ids come from: the fields MotByteFcMixDesc, MotByteCatDesc, MotValueMixDesc and MotSplitX0Desc share.
struct IdSource {
    const int32_t *tokens;
    int64_t n_rows, tokens_per_row;
    int bpt, id_source, pull_dir;
    const void *ttb;
    int64_t ttb_rows;
    int ttb_elem_bytes;
    const int64_t *ids;
    int32_t pad_byte, eot_byte;
    int64_t *out_ids_padded, *out_ids_pulled, *counters;
    uint32_t *status;
};
template <class Desc>
inline IdSource id_source_of(const Desc &d) {
    return {d.tokens, d.n_rows, d.tokens_per_row, d.bpt, d.id_source, d.pull_dir, d.ttb, d.ttb_rows, d.ttb_elem_bytes,
            d.ids, d.pad_byte, d.eot_byte, d.out_ids_padded, d.out_ids_pulled, d.counters, d.status};
}
inline IdSource id_source_of(const MotValueMixDesc &d) {   // one id output (the ids the call used), no statistics
    return {d.tokens, d.n_rows, d.tokens_per_row, d.bpt, d.id_source, d.pull_dir, d.ttb, d.ttb_rows, d.ttb_elem_bytes,
            d.ids, d.pad_byte, d.eot_byte, nullptr, d.out_ids, nullptr, d.status};
}

// The shape checks of the id source; `fn` is the message prefix.  Two functions, because every front-end checks its own tables
// and widths between them and the first refusal is the one the caller reads.
inline int check_id_source_shape(const char *fn, const IdSource &s, bool backward) {
    if (s.bpt < 1 || s.bpt > MOT_MAX_BPT) return set_error(MOT_EUNSUPPORTED, "%s: bytes_per_token %d outside [1, %d]", fn, s.bpt, MOT_MAX_BPT);
    if (s.id_source == MOT_IDS_FROM_TTB) {
        if (s.ttb_elem_bytes != 2 && s.ttb_elem_bytes != 4) return set_error(MOT_EINVAL, "%s: ttb_elem_bytes must be 2 or 4", fn);
        if (s.pull_dir < MOT_PULL_NONE || s.pull_dir > MOT_PULL_RIGHT) return set_error(MOT_EINVAL, "%s: bad pull_dir %d", fn, s.pull_dir);
        if (s.ttb_rows <= 0) return set_error(MOT_EINVAL, "%s: ttb missing", fn);
        if (backward) return set_error(MOT_EUNSUPPORTED, "%s_bwd: pass the byte ids the forward used (MOT_IDS_GIVEN)", fn);
    } else if (s.id_source != MOT_IDS_GIVEN) {
        return set_error(MOT_EINVAL, "%s: bad id_source %d", fn, s.id_source);
    }
    return MOT_OK;
}
inline int check_id_source_limits(const char *fn, const IdSource &s) {
    if (s.tokens_per_row * (int64_t)s.bpt > 0x7fffffffLL || s.n_rows * s.tokens_per_row > 0x7fffffffLL)
        return set_error(MOT_EUNSUPPORTED, "%s: T*bpt or B*T exceeds 2^31", fn);
    return MOT_OK;
}
// the pointers of the id source; `outs` names the id outputs in the message
inline int check_id_source_ptrs(const char *fn, const IdSource &s, const char *outs = "out_ids_* need") {
    if (s.id_source == MOT_IDS_FROM_TTB) {
        if (!s.ttb) return set_error(MOT_EINVAL, "%s: ttb missing", fn);
    } else {
        if (!s.ids) return set_error(MOT_EINVAL, "%s: ids missing", fn);
        if (s.out_ids_padded || s.out_ids_pulled) return set_error(MOT_EINVAL, "%s: %s MOT_IDS_FROM_TTB", fn, outs);
    }
    return MOT_OK;
}
inline int check_workspace(const char *fn, bool backward, const void *ptr, size_t have, size_t need) {
    if (need && (!ptr || have < need || ((uintptr_t)ptr & 15)))
        return set_error(MOT_EWORKSPACE, "%s%s: needs %zu 16-byte aligned workspace bytes, got %zu", fn, backward ? "_bwd" : "", need, have);
    return MOT_OK;
}

// The byte ids from the token->byte table with the loader's two index kernels: tokens_to_bytes into `padded`, then the pull (if
// there is one) into `pulled`.  The caller chooses the two buffers (its id outputs or its workspace); *ids is what the call reads.
inline int launch_ids_from_ttb(const IdSource &s, int64_t *padded, int64_t *pulled, const int64_t **ids, hipStream_t stream) {
    if (int rc = launch_tokens_to_bytes(s.tokens, s.n_rows * s.tokens_per_row, s.ttb, s.ttb_elem_bytes, s.ttb_rows, s.bpt, padded, s.status, stream)) return rc;
    *ids = padded;
    if (s.pull_dir == MOT_PULL_NONE) return MOT_OK;
    *ids = pulled;
    return launch_pull_bytes(padded, pulled, s.n_rows, s.tokens_per_row, s.bpt, s.pad_byte, s.eot_byte, s.pull_dir == MOT_PULL_LEFT ? kPullLeft : kPullRight,
                             stream);
}

}  // namespace mot
