/*
 * mot.h -- C ABI of libmot_hip.so: the MI355X (gfx950) implementation of the
 * mixture-of-tokenizers embedding front-end.
 *
 * The reference (snimu/mixture-of-tokenizers) exposes this path as Python functions and
 * nn.Module.forward() calls, not as an FFI; each entry point below names the reference
 * interface it replaces (paths relative to the reference checkout).  Host bindings live in
 * mixture-of-tokenizers_amd/_capi.py (ctypes); INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless a comment says "host"
 *   - the caller owns all buffers (inputs, outputs, workspace); the library allocates nothing and
 *     reads no environment variable; every choice between kernels is a field of the descriptor
 *     (MotEmbedMixDesc.flags).  The only thing it remembers between calls is, per device, which
 *     kernels already had their dynamic-LDS limit raised (hipFuncSetAttribute, idempotent), so
 *     calls are re-entrant and hipGraph-capturable
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and never synchronises the host
 *   - return value: MOT_OK or a negative MotStatus; mot_last_error() gives a thread-local
 *     message for the last failing call on this thread
 *   - byte tensors use the reference's layout: (B, T*bpt) row-major, token-major / slot-minor
 */
#ifndef MOT_H_
#define MOT_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOT_ABI_VERSION 13
#define MOT_MAX_BPT 64 /* bytes (characters) per token; the reference uses 3, 8, 16, 18, 20, 32 */

typedef void *mot_stream_t; /* hipStream_t */

typedef enum MotStatus {
    MOT_OK = 0,
    MOT_EINVAL = -1,       /* null pointer / bad enum / bad struct_size                     */
    MOT_ESHAPE = -2,       /* shape the reference asserts on (e.g. T % bytes_per_token)     */
    MOT_EUNSUPPORTED = -3, /* valid request this build has no kernel for                    */
    MOT_EHIP = -4,         /* HIP runtime error (launch failure, no device)                 */
    MOT_EWORKSPACE = -5    /* workspace missing or smaller than mot_embed_mix_workspace_bytes */
} MotStatus;

/* Bits of the optional device status word (`status` arguments / MotEmbedMixDesc.status).
 * Kernels OR them in with atomics; out-of-range ids are clamped to row 0 so that a bad id can
 * never fault -- the host shim turns a non-zero word into the reference's IndexError. */
#define MOT_STATUS_TOKEN_OOR 1u /* token id outside [0, tok_rows) / [0, ttb_rows) */
#define MOT_STATUS_BYTE_OOR 2u  /* byte id outside [0, byte_rows)                 */
#define MOT_STATUS_TARGET_OOR 4u /* target outside [0, vocab) (mot_byte_head_*, mot_token_head_*, mot_plain_head_*) */
#define MOT_STATUS_KEPT_OVERFLOW 8u /* more kept rows than max_kept (mot_plain_head_compact_*): nothing was scored */
#define MOT_STATUS_LOGIT_NONFINITE 16u /* a row of mot_next_token held a NaN or +inf logit: its token is -1 */

typedef enum MotPullDir {
    MOT_PULL_NONE = 0,
    MOT_PULL_LEFT = 1, /* pull_from_left : window ends at the token, right-aligned  */
    MOT_PULL_RIGHT = 2 /* pull_from_right: window starts at the token, left-aligned */
} MotPullDir;

typedef enum MotMixMode {
    MOT_MIX_NOOP = 0,         /* x = tok part            (train_gpt.py:342-348, 421-427)            */
    MOT_MIX_SUM = 1,          /* x = a + concat_k b_k    (modded-nanogpt/runs/71_*.py:227-230)      */
    MOT_MIX_MEAN = 2,         /* x = a + mean_k b_k      (inference/inference.py:266-267)           */
    MOT_MIX_CONCAT_LINEAR = 3, /* x = W.cat(a, b_*) + bias (train_gpt.py:430-443; model.py:256-268) */
    MOT_MIX_CONCAT = 4        /* x = cat(a, b_*): "MoT via pure concatenation", no weight, no GEMM
                                 (modded-nanogpt/runs/711_*.py:224-232, call site 314-316; runs 712, 713) */
} MotMixMode;

typedef enum MotIdSource {
    MOT_IDS_NONE = 0,     /* MOT_MIX_NOOP                                                       */
    MOT_IDS_FROM_TTB = 1, /* fully fused: tokens -> ttb gather -> pull, byte ids never leave LDS */
    MOT_IDS_GIVEN = 2     /* ids_a (and ids_b) precomputed int64, as the reference loader emits  */
} MotIdSource;

/* Element type of the tables, the weight and `out` (scalars, workspace and gradients stay fp32).
 * MOT_BF16 is what the production loop runs (nn.Embedding -> bf16, train_gpt.py:1124-1126): rows are
 * widened to fp32 on load, all arithmetic is fp32, results are rounded once (nearest-even) on store;
 * eps defaults to torch.finfo(bfloat16).eps = 2^-7, as F.rms_norm(eps=None) does on bf16 inputs. */
typedef enum MotDType { MOT_F32 = 0, MOT_BF16 = 1 } MotDType;

int mot_version(void);                /* MOT_ABI_VERSION the library was built with */
const char *mot_last_error(void);     /* host string, thread-local, never NULL      */
const char *mot_build_info(void);     /* host string: arch, compiler, build flags   */

/*
 * Replaces tokens_to_bytes(tokens, emb)           scaled-pre-train/data_creation.py:61-67
 * (and the table built by make_embedding, :51-58, which the host keeps as an integer table).
 *   tokens  int32 [n_tokens]         ttb  int16|int32 [ttb_rows, bpt] (ttb_elem_bytes = 2|4)
 *   out     int64 [n_tokens*bpt]     status optional
 */
int mot_tokens_to_bytes(const int32_t *tokens, int64_t n_tokens, const void *ttb,
                        int ttb_elem_bytes, int64_t ttb_rows, int bpt, int64_t *out,
                        uint32_t *status, mot_stream_t stream);

/*
 * Replaces pull_from_left / pull_from_right(byte_tensor, bytes_per_token, pad_byte, eot_byte)
 *                                                 scaled-pre-train/data_creation.py:179-305 / 71-176
 *   in, out  int64 [B, T] with T = tokens_per_row*bpt; any int64 values are legal
 *   T == 0 is a no-op (data_creation.py:82-83,190); T % bpt != 0 -> MOT_ESHAPE (:85,192)
 *   in == out is NOT allowed.
 */
int mot_pull_bytes(const int64_t *in, int64_t *out, int64_t B, int64_t T, int bpt,
                   int64_t pad_byte, int64_t eot_byte, int dir /* MotPullDir */,
                   mot_stream_t stream);

/*
 * Replaces create_batch(tokens, bpt, pad, eot, ttb_right, ttb_left)
 *                                                 scaled-pre-train/data_creation.py:308-330
 *   out int64 [B, T, 1 + 4*bpt] = [token | left-padded | pulled-from-left | right-padded |
 *   pulled-from-right]; one fused launch, no intermediate tensors.
 */
int mot_create_batch(const int32_t *tokens, int64_t B, int64_t T, const void *ttb_left,
                     const void *ttb_right, int ttb_elem_bytes, int64_t ttb_rows, int bpt,
                     int64_t pad_byte, int64_t eot_byte, int64_t *out, uint32_t *status,
                     mot_stream_t stream);

/*
 * Replaces TokenMixByCharStreamingDataset.chr_tokenize + create_char_matrix     inference/inference.py:56-67, 79-96
 * (the producer of the character ids of BASELINE config 5; a host-side Python loop in the reference), for a batch of
 * sequences in one launch.
 *   seq_offsets int64 [n_seqs + 1]: entries (one per BPE token, in order) of sequence s are [seq_offsets[s], seq_offsets[s+1])
 *   tok_offsets int64 [n_entries + 1]: code points of entry e are codes[tok_offsets[e] .. tok_offsets[e+1])
 *   codes       int32: Unicode code points of the token strings (chr_tokenize's `ord(x)`); a NEGATIVE value c is a literal
 *               character id -c - 1 (the [129] row get_tokens prepends for BOS, line 73, is passed as -130)
 *   out         int64 [n_seqs, seq_len, max_char]: ids 0-127 ASCII, 128 the tokenizer's leading-space marker, 129 / 130 a
 *               code point equal to the BOS / EOS token id (the reference compares ord(x) with the TOKEN ids, lines 62-65),
 *               131 any other character; one end-of-word 130 after the last character of a row that is not full; 2 elsewhere
 *               (line 82) and on rows past the sequence's entries; characters beyond max_char are dropped (lines 89-91).
 */
int mot_char_matrix(const int32_t *codes, const int64_t *tok_offsets, const int64_t *seq_offsets, int64_t n_seqs,
                    int64_t seq_len, int max_char, int32_t leading_space, int32_t bos_token_id, int32_t eos_token_id,
                    int64_t *out, mot_stream_t stream);

/*
 * Replaces emb(ids) / norm(emb(ids)) / norm(emb(ids_a) + emb(ids_b)) when the caller wants the
 * tensors at the FlexibleEmbedding seam materialised
 *                                                 scaled-pre-train/train_gpt.py:342-379, 172-173
 *   ids int64|int32 [n] (ids_elem_bytes 8|4), ids_b optional; table f32|bf16 [rows, dim];
 *   out (same type) [n, dim]; rms_norm: x * rsqrt(mean(x^2) + eps), eps <= 0 -> FLT_EPSILON
 *   (F.rms_norm eps=None); scale optional device scalar.
 */
int mot_gather_rows(const void *ids_a, const void *ids_b, int ids_elem_bytes, int64_t n,
                    const void *table, int64_t rows, int dim, int rms_norm, float eps,
                    const float *scale, void *out, uint32_t *status, int dtype /* MotDType */,
                    mot_stream_t stream);

/*
 * The fused front-end.  Replaces, in ONE launch (plus a 458-row prologue when norm_byte is set):
 *   FlexibleEmbedding.forward + ByteMixin.forward  scaled-pre-train/train_gpt.py:327-379, 421-480
 *   (call site train_gpt.py:605-606), optionally with the loader's tokens_to_bytes + pull
 *   (train_gpt.py:686-728) folded in;
 *   GPT.wte / GPT.dte / digit_mixin                mathblations/model.py:256-268, 304-306, 323-327;
 *   embed_tokens / embed_bytes / mixin_bytes       modded-nanogpt/runs/71_*.py:227-230, 312-314
 *   (and the per-embedding-norm / lambda variants runs/71041_*.py:311-313, runs/71081_*.py:302-315);
 *   mixin_bytes of the pure-concatenation runs      modded-nanogpt/runs/711_*.py:224-232, 314-316
 *   (MOT_MIX_CONCAT: x = [a | b_0 | .. | b_{bpt-1}], model_dim = tok_dim + bpt*byte_dim; tok_dim and byte_dim multiples of the
 *   16-byte vector, 4 fp32 / 8 bf16 elements, so that no vector straddles two parts; no weight, no bias; norm_tok is over the tok_dim
 *   columns, norm_out over all model_dim; with two id tensors b_k = E[idsA] + E[idsB], normalised as a sum when norm_byte is set,
 *   which needs byte_dim = vector * 2^k and tok_dim a multiple of byte_dim).
 *
 * Per token n of row-major (B, T):
 *   a   = tok_table[tokens[n]];            if norm_tok:  a = rms_norm(a);    a *= *scale_tok
 *   b_k = byte_table[idsA[n,k]] (+ byte_table[idsB[n,k]]);
 *                                          if norm_byte: b_k = rms_norm(b_k); b_k *= *scale_byte
 *   x   = mix(a, b_0..b_{bpt-1}) per `mode`;  if norm_out: x = rms_norm(x)
 * where idsA/idsB come from `id_source`:
 *   MOT_IDS_FROM_TTB: padded = ttb[tokens[n]], pulled = pull(padded) along each row;
 *       idsA = pulled (or padded when pull_dir == NONE); idsB = padded iff add_padded
 *   MOT_IDS_GIVEN:    idsA = ids_a, idsB = ids_b (NULL = none)
 */
/* MotEmbedMixDesc.flags: kernel selection, resolved by the caller once (the Python shim reads its own switches at
 * import); results agree to the parity bar either way, the workspace size may differ -- size it with the same flags. */
#define MOT_FLAG_LINEAR_ONE_LAUNCH 1u /* CONCAT_LINEAR: the one-launch tile kernel instead of the composed kernels       */
#define MOT_FLAG_MEAN_GENERIC 2u      /* MEAN: the whole-row kernel even where the LDS column-slice kernel qualifies     */
#define MOT_FLAG_BWD_DU_FP32 4u       /* CONCAT_LINEAR backward, bf16: du = dy.W on the fp32 MFMA instead of the bf16 one */
#define MOT_FLAG_LINEAR_COMPOSED 8u   /* CONCAT_LINEAR, bf16: the multi-kernel path even where the one gather-GEMM qualifies */

typedef struct MotEmbedMixDesc {
    uint32_t struct_size; /* sizeof(MotEmbedMixDesc), checked */
    int32_t dtype;        /* MotDType of tables / weight / out */
    uint32_t flags;       /* MOT_FLAG_* */
    uint32_t reserved0;   /* must be 0 */

    /* problem */
    int64_t n_rows;         /* B */
    int64_t tokens_per_row; /* T (tokens, not byte slots) */
    int32_t bpt;            /* byte slots per token; 0 for MOT_MIX_NOOP */
    int32_t mode;           /* MotMixMode */

    /* ids */
    const int32_t *tokens; /* [B, T] */
    int32_t id_source;     /* MotIdSource */
    int32_t pull_dir;      /* MotPullDir          (FROM_TTB) */
    const void *ttb;       /* [ttb_rows, bpt]     (FROM_TTB) */
    int64_t ttb_rows;
    int32_t ttb_elem_bytes; /* 2 | 4 */
    int32_t add_padded;     /* FROM_TTB: idsB = unpulled row (train_gpt.py:371-379) */
    int32_t pad_byte, eot_byte;
    const int64_t *ids_a; /* [B, T*bpt]          (GIVEN) */
    const int64_t *ids_b; /* optional            (GIVEN) */

    /* tables */
    const void *tok_table; /* [tok_rows, tok_dim], contiguous */
    int64_t tok_rows;
    int32_t tok_dim;
    int32_t byte_dim;
    const void *byte_table; /* [byte_rows, byte_dim] */
    int64_t byte_rows;

    /* mixing */
    int32_t model_dim;   /* output columns; SUM/MEAN/NOOP require == tok_dim, CONCAT == tok_dim + bpt*byte_dim */
    int32_t bytes_first; /* CONCAT_LINEAR: 0 = [a, b_*] (train_gpt.py:443), 1 = [b_*, a] (model.py:267) */
    const void *weight;  /* CONCAT_LINEAR: [model_dim, tok_dim + bpt*byte_dim] row-major (nn.Linear) */
    const void *bias;    /* optional [model_dim] */
    int32_t norm_tok, norm_byte, norm_out;
    float eps;                /* <= 0 -> FLT_EPSILON (torch.finfo(float32).eps) */
    const float *scale_tok;   /* optional device scalar */
    const float *scale_byte;  /* optional device scalar */

    /* outputs */
    void *out;               /* [B, T, model_dim] */
    int64_t *out_ids_padded; /* optional [B, T*bpt]: what tokens_to_bytes would return (FROM_TTB) */
    int64_t *out_ids_pulled; /* optional [B, T*bpt]: what pull_from_* would return    (FROM_TTB) */
    int64_t *counters;       /* optional int64[4], atomically incremented: tokens, byte slots,
                                pads before the pull, pads after (runs/79_*.py:484-488)        */
    uint32_t *status;        /* optional device word, see MOT_STATUS_* */
    float *out_row_rnorm;    /* optional [B, T] fp32: rsqrt(mean(y^2)+eps) of every output row when norm_out
                                (CONCAT_LINEAR); saved by autograd so the backward need not redo the GEMM */

    /* scratch */
    void *workspace; /* >= mot_embed_mix_workspace_bytes(desc); may be NULL when that is 0 */
    size_t workspace_bytes;
} MotEmbedMixDesc;

/*
 * Backward of mot_embed_mix_fwd: replaces what autograd does for the modules above when the
 * training loop calls loss.backward() (scaled-pre-train/train_gpt.py:1319; mathblations/main.py:304).
 * `fwd` is the forward's descriptor with id_source == MOT_IDS_GIVEN (pass the byte ids the forward
 * returned through out_ids_*); `out`, `out_ids_*`, `counters` are ignored.  Gradients are ACCUMULATED
 * (+=) into the given buffers, so a parameter's .grad can be passed directly; NULL = not wanted.
 * Built: MOT_MIX_SUM, MOT_MIX_NOOP, MOT_MIX_CONCAT, MOT_MIX_CONCAT_LINEAR, and MOT_MIX_MEAN without an output norm (the residual of
 * inference.py:267 has none; its small character table makes the table gradient a dense product, mot_bwd_mean.hip; with
 * bf16 tables that product runs on operands widened slab by slab into the workspace).
 * With dtype == MOT_BF16 the tables, weight/bias, `out` and grad_out are bf16 as in the forward, while
 * every gradient buffer below stays FP32 (sums of thousands of terms are accumulated in fp32; the
 * caller rounds once when it needs a bf16 .grad, train_gpt.py:1124-1126).
 * CONCAT_LINEAR additionally needs `out` (the forward's x) and, when norm_out, `out_row_rnorm` of the
 * forward in `fwd`, and a workspace of mot_embed_mix_bwd_workspace_bytes(fwd).
 * Sums use float atomics: results are order-dependent in the last bits, like the reference's own
 * GPU embedding backward.
 */
typedef struct MotEmbedMixGrads {
    uint32_t struct_size;  /* sizeof(MotEmbedMixGrads) */
    uint32_t reserved;
    const void *grad_out;  /* [B, T, model_dim] upstream gradient dL/dx */
    void *d_tok_table;     /* [tok_rows, tok_dim]   fp32 */
    void *d_byte_table;    /* [byte_rows, byte_dim] fp32 */
    void *d_weight;        /* [model_dim, K]   fp32 (CONCAT_LINEAR) */
    void *d_bias;          /* [model_dim]      fp32 (CONCAT_LINEAR with bias; optional) */
    float *d_scale_tok;    /* scalar */
    float *d_scale_byte;   /* scalar */
    const int32_t *token_order; /* optional: what mot_token_order wrote for fwd->tokens (same n_tokens, tok_rows); NULL = the
                                   backward groups the positions itself, inside its workspace */
} MotEmbedMixGrads;

/*
 * The grouping of a batch's positions by token id that the table-gradient scatter walks (a counting sort: three small kernels,
 * 0.08 ms at 256 x 2048 tokens).  It depends on `tokens` only -- not on the tables, not on grad_out -- so a caller can produce it
 * once per batch, e.g. beside the forward (the Python autograd node runs it on a side stream while the forward streams), and hand
 * it to every backward over the same tokens through MotEmbedMixGrads.token_order (several embedding tables indexed by one
 * token tensor: modded-nanogpt/runs/71_*.py value embeddings; gradient accumulation does not re-sort either).
 *   tokens int32 [n_tokens]; ids outside [0, tok_rows) are flagged in `status` and grouped under row 0 (as the backward does);
 *   order  int32 [mot_token_order_ints(n_tokens, tok_rows)], opaque.  tok_rows < 2^21 - 1, n_tokens < 2^31.
 */
size_t mot_token_order_ints(int64_t n_tokens, int64_t tok_rows);
int mot_token_order(const int32_t *tokens, int64_t n_tokens, int64_t tok_rows, int32_t *order, uint32_t *status,
                    mot_stream_t stream);

size_t mot_embed_mix_bwd_workspace_bytes(const MotEmbedMixDesc *fwd /* host */);
int mot_embed_mix_bwd(const MotEmbedMixDesc *fwd /* host */, const MotEmbedMixGrads *grads /* host */,
                      mot_stream_t stream);

/*
 * The write-once backward of mot_embed_mix_fwd (opt-in; mot_embed_mix_bwd above is unchanged).  `fwd` as for mot_embed_mix_bwd
 * (id_source == MOT_IDS_GIVEN), with a workspace of mot_embed_mix_bwd_once_workspace_bytes(fwd).
 *   d_tok_table[r, :] = round_to_dtype(sum over the positions p with tokens[p] == r of d a_p): the sum in fp32 in ascending
 *   position order (cut at multiples of 64 sorted slots; the pieces of a group that crosses a cut in ascending slice order, in
 *   four fixed quarters), rounded once, +0 where r does not occur.  EVERY element is written exactly once: the caller zeroes
 *   nothing, no atomic touches a gradient element, and the same call gives the same bits -- with a caller's token_order or one made
 *   in the call, eagerly or replayed from a graph (no memset or memcpy node is used).
 *   d_byte_table (fp32) is cleared by the call with a kernel and then summed in 64-bit fixed point (integer atomics in LDS and
 *   global memory: the sums do not depend on the order of the adds), slab by slab of 16 384 positions;
 *   d_scale_tok / d_scale_byte (fp32) are written, summed in a fixed order.
 * With dtype == MOT_BF16 the forward quantities are recomputed from the tables in fp32 and are not re-rounded.
 * Built: MOT_MIX_SUM, MOT_MIX_NOOP, MOT_MIX_CONCAT; fp32 and bf16; one id tensor; every norm / scale combination that
 * mot_embed_mix_bwd takes for those modes; tok_dim and byte_dim multiples of the 16-byte vector, model_dim <= 2048,
 * tok_rows < 2^21 - 1.  MOT_MIX_CONCAT_LINEAR, MOT_MIX_MEAN, ids_b and MOT_IDS_FROM_TTB return MOT_EUNSUPPORTED before any HIP call
 * (the message starts "embed_mix_bwd_once" and names the follow-up); a missing or short workspace MOT_EWORKSPACE; null pointers and a
 * bad struct_size MOT_EINVAL; an empty batch MOT_OK without a launch.  Out-of-range ids are clamped to row 0 and flagged in
 * fwd->status.  No piece of the workspace is proportional to n_tokens x model_dim: it holds the token order and the canonical
 * positions, 16 bytes of scalars per position, the slice pieces and ONE slab (16 384 positions) of the byte part's fp32 rows.
 */
typedef struct MotEmbedMixGradsOnce {
    uint32_t struct_size; /* sizeof(MotEmbedMixGradsOnce) */
    uint32_t reserved;    /* must be 0 */
    const void *grad_out; /* [B, T, model_dim] in fwd->dtype */
    void *d_tok_table;    /* [tok_rows, tok_dim] in fwd->dtype, WRITTEN (every element, once); NULL = not wanted */
    float *d_byte_table;  /* [byte_rows, byte_dim] fp32, OVERWRITTEN (the call clears it with a kernel); NULL = not wanted */
    float *d_scale_tok;   /* fp32 scalar, WRITTEN; NULL = not wanted */
    float *d_scale_byte;  /* fp32 scalar, WRITTEN; NULL = not wanted */
    const int32_t *token_order; /* optional, as in MotEmbedMixGrads */
} MotEmbedMixGradsOnce;
size_t mot_embed_mix_grads_once_size(void); /* sizeof(MotEmbedMixGradsOnce) in this build, for bindings */
size_t mot_embed_mix_bwd_once_workspace_bytes(const MotEmbedMixDesc *fwd /* host */); /* 0 for a descriptor the call would refuse */
int mot_embed_mix_bwd_once(const MotEmbedMixDesc *fwd /* host */, const MotEmbedMixGradsOnce *grads /* host */, mot_stream_t stream);

/*
 * CONCAT_LINEAR runs as several kernels inside one call (index kernels when the ids come from the ttb, a gather that
 * writes the concat operand into the workspace, a dense MFMA kernel, a row-norm pass); in bf16, with one id tensor, embedding
 * dims that are multiples of 8, a concat width that is a multiple of 32 and model_dim 256/512/768/1024, everything behind the
 * index kernels is ONE gather-GEMM kernel (MOT_FLAG_LINEAR_COMPOSED keeps the separate kernels).  MOT_FLAG_LINEAR_ONE_LAUNCH in
 * desc->flags selects the older one-launch tile kernel instead.  Same results to the parity bar; the workspace size differs,
 * so mot_embed_mix_workspace_bytes must see the same flags as the call.
 */
size_t mot_embed_mix_desc_size(void); /* sizeof(MotEmbedMixDesc) in this build, for bindings */
size_t mot_embed_mix_workspace_bytes(const MotEmbedMixDesc *desc /* host */);
int mot_embed_mix_fwd(const MotEmbedMixDesc *desc /* host */, mot_stream_t stream);

/*
 * Cross-attention byte mixin, forward: replaces ByteMixinCrossAttn.forward on FlexibleEmbedding's outputs
 * (scaled-pre-train/train_gpt.py:446-464 -> CrossAttention.forward 271-300; embeddings 342-379).
 * Each token attends to its own `bpt` byte embeddings: q = q_w xq, (k, v) = kv_w xkv, per-head rms-norm of q and
 * k, RoPE with the position in each one's own sequence, v *= lambda, softmax(q.k / sqrt(hd)) over the bpt
 * keys, out = proj_w y.  The reference asserts batch 1 (line 275): tokens is one row of n_tokens.
 * head_dim is 128 (line 459); dim = token_dim = byte_dim = model_dim (line 449).  fp32.
 * head_layout MOT_HEADS_AS_VIEWED reproduces lines 283-284 (k, v are reshaped, not transposed, into
 * (H, T, bpt, hd)); MOT_HEADS_PER_TOKEN is the einops expression in the comment of those lines.
 * cos/sin are the Rotary buffers of the module (lines 190-197), fp32 [len, 64], built by the caller.
 */
typedef enum MotHeadLayout { MOT_HEADS_AS_VIEWED = 0, MOT_HEADS_PER_TOKEN = 1 } MotHeadLayout;

typedef struct MotCrossAttnDesc {
    uint32_t struct_size;     /* sizeof(MotCrossAttnDesc) */
    int32_t dtype;            /* MOT_F32 */
    int64_t n_tokens;         /* Tq; Tkv = n_tokens * bpt */
    int32_t bpt;              /* chars_per_token, line 282 */
    int32_t n_heads;          /* hdim = n_heads * 128 */
    int32_t head_layout;      /* MotHeadLayout */
    int32_t dim;              /* columns of both tables */
    const int32_t *tokens;    /* [n_tokens] */
    const int64_t *ids_a;     /* [n_tokens * bpt] byte ids */
    const int64_t *ids_b;     /* optional second id tensor: xkv = norm?(E[a] + E[b]), line 378 */
    const void *tok_table;    /* [tok_rows, dim] */
    int64_t tok_rows;
    const void *byte_table;   /* [byte_rows, dim] */
    int64_t byte_rows;
    int32_t norm_tok;         /* FlexibleEmbedding applies norm() to both (lines 367-378) */
    int32_t norm_byte;
    const void *q_w;          /* [hdim, dim]    CrossAttention.q_w */
    const void *kv_w;         /* [2, hdim, dim] CrossAttention.kv_w */
    const void *proj_w;       /* [dim, hdim]    CrossAttention.c_proj.weight */
    const float *lambda_factor; /* device scalar */
    const float *cos_q, *sin_q; /* [>= n_tokens, 64] */
    const float *cos_k, *sin_k; /* [>= n_tokens * bpt, 64] */
    int64_t rot_q_len, rot_k_len; /* rows of the two pairs of buffers (line 200 asserts they suffice) */
    float eps;                /* 0 = finfo(float32).eps */
    int32_t kv_tables_ready;  /* forward, one id tensor: 1 = `kv_tables` already holds this call's tables (skip building them) */
    void *out;                /* [n_tokens, dim] */
    uint32_t *status;         /* optional, as in MotEmbedMixDesc */
    void *workspace;          /* mot_cross_attn_workspace_bytes(desc) */
    size_t workspace_bytes;
    /* optional, forward with one id tensor: caller-kept buffer of 2 * byte_rows * n_heads * 128 floats for the per-byte-row
     * key / value tables.  They depend on byte_table, kv_w and lambda_factor only, so an inference loop builds them once:
     * pass the buffer with kv_tables_ready = 0 after those change (the call fills it), = 1 otherwise. */
    void *kv_tables;
    /* optional: buffer of 2 * n_tokens * n_heads * 128 floats.  The forward leaves the projected queries and the attention
     * output there; the backward, given the same buffer, reads them instead of recomputing that part of the forward. */
    void *saved_qy;
    /* MOT_F32 (0) or MOT_BF16: where the products over the tokens run (q = W_q xq, out = c_proj y; backward: dW_p, dy, dW_q, dxq).
     * MOT_BF16 = the bf16 MFMA with fp32 accumulation: their row operands (xq, y, grad_out, dq) are rounded to bf16 first and the
     * weights are taken as bf16 -- the values those operands have in the reference's production cast (CastedLinear and
     * `self.q_w.type_as(x)`, train_gpt.py:185-186, 277-278; x bf16 since 1124-1126).  With one id tensor and bpt <= 16 the attention
     * kernels also read norm(k) and lambda * v from bf16 copies of the two per-row tables (bf16 tensors in that cast, lines 278, 280);
     * the attention arithmetic, the tables themselves and every gradient stay fp32.  Needs dim % 8 == 0.  Workspace sizes depend on it. */
    int32_t matmul_dtype;
    /* MOT_F32 (0) or, with matmul_dtype == MOT_BF16, MOT_BF16: the element type of `out` (forward) and of MotCrossAttnGrads.grad_out
     * (backward).  bf16 is what the reference's module returns and receives in the production cast; the last product then writes
     * bf16 itself (one rounding of the fp32 sums, as a caller's cast of the fp32 result would do) and the backward's bf16 products
     * take grad_out as it is -- a widening and a narrowing pass over [T, dim] less on each side of the boundary. */
    int32_t io_dtype;
    /* optional, with matmul_dtype == MOT_BF16: the caller's bf16 token table [tok_rows, dim] whose widened copy `tok_table` is.
     * The normalised token rows -- the row operand of W_q and of dW_q -- are then gathered in bf16 directly (the same values: norm
     * in fp32, one rounding), without the fp32 detour. */
    const void *tok_table_bf16;
} MotCrossAttnDesc;

/*
 * Backward of mot_cross_attn_fwd (loss.backward() through the modules above, train_gpt.py:1319).  `fwd` is the
 * forward's descriptor (`out` is ignored); everything is recomputed from the inputs.  Gradients are ACCUMULATED (+=)
 * in fp32 into the given buffers.  With two id tensors (ids_b, the add_padded_and_pulled embedding of train_gpt.py:364-372)
 * the key / value rows are per kv position: the workspace then grows with n_tokens * bpt rows of 2 * heads * 128 floats.
 */
typedef struct MotCrossAttnGrads {
    uint32_t struct_size;  /* sizeof(MotCrossAttnGrads) */
    uint32_t reserved;
    const void *grad_out;  /* [n_tokens, dim] */
    void *d_tok_table;     /* [tok_rows, dim]  */
    void *d_byte_table;    /* [byte_rows, dim] */
    void *d_q_w;           /* [hdim, dim]      */
    void *d_kv_w;          /* [2, hdim, dim]   */
    void *d_proj_w;        /* [dim, hdim]      */
    float *d_lambda;       /* scalar           */
} MotCrossAttnGrads;

size_t mot_cross_attn_bwd_workspace_bytes(const MotCrossAttnDesc *fwd /* host */);
int mot_cross_attn_bwd(const MotCrossAttnDesc *fwd /* host */, const MotCrossAttnGrads *grads /* host */, mot_stream_t stream);

size_t mot_cross_attn_desc_size(void);
size_t mot_cross_attn_workspace_bytes(const MotCrossAttnDesc *desc /* host */);
int mot_cross_attn_fwd(const MotCrossAttnDesc *desc /* host */, mot_stream_t stream);

/*
 * Sliding-window token <- character attention of the Llama character mixer, forward: replaces
 *   TokenMixByCharBMM.forward                      inference/inference.py:146-224  (swa_transform 174-179)
 *   the residuals of TokenMixByCharBMMBlock.forward                       :260-267 (the SwiGLU feed-forward after them, 269, is
 *   a plain MLP and stays with the caller) on top of the gathers of CustomLlamaModel.forward, :323-327.
 * Per token t of row-major (B, T):  xn = RMSNorm_a(E_tok[t]), cn = RMSNorm_c(E_char[c]) (x * rsqrt(mean(x^2) + norm_eps) * weight,
 * lines 126-132), q = wq xn, keys / values = wk cn / wv cn of the c_v characters of each of the tokens t-window+1 .. t of the
 * token's batch row (zero vectors in front of the row: they keep their place in the softmax with score 0), rotary embedding of
 * q and of every key at the query's position (see mot_swa.hip: it cancels), p = softmax(q . k / sqrt(head_dim)), y = sum p v,
 * out = wo y  (+ toks  |  + lambda_tok toks + lambda_char mean_c chars).   fp32; head_dim 64 or 128; window * c_v <= 64.
 * The reference cannot be imported offline (hub login at import): PARITY UNPINNED, checked against a hand-written float64 restatement.
 */
typedef enum MotSwaVersion { MOT_SWA_NO_RESIDUAL = 0, MOT_SWA_ONE_RESIDUAL = 1, MOT_SWA_TWO_RESIDUAL = 2 } MotSwaVersion;

typedef struct MotCharSwaDesc {
    uint32_t struct_size;       /* sizeof(MotCharSwaDesc) */
    int32_t dtype;              /* MOT_F32 */
    int64_t n_rows;             /* B */
    int64_t tokens_per_row;     /* T */
    int32_t c_v;                /* characters per token (max_char, 8) */
    int32_t window;             /* TokenMixByCharBMM.window_size (8) */
    int32_t n_heads, head_dim;  /* ModelArgs.n_heads, head_dim (32 x 64 for Llama-3.2-1B) */
    int32_t dim;                /* ModelArgs.dim: columns of both tables and of out */
    int32_t version;            /* MotSwaVersion */
    const int32_t *tokens;      /* [B, T] */
    const int64_t *char_ids;    /* [B, T, c_v] */
    const void *tok_table;      /* [tok_rows, dim]  model.embed_tokens.weight */
    int64_t tok_rows;
    const void *char_table;     /* [char_rows, dim] char_embeddings.weight */
    int32_t char_rows;          /* 132 */
    float norm_eps;             /* <= 0 -> 1e-5 (ModelArgs.norm_eps) */
    const void *attn_norm_w;    /* [dim] attention_norm.weight */
    const void *char_norm_w;    /* [dim] char_norm.weight */
    const void *wq, *wk, *wv;   /* [n_heads * head_dim, dim] nn.Linear weights, no bias */
    const void *wo;             /* [dim, n_heads * head_dim] */
    const float *lambda_tok;    /* device scalars (two_residual); NULL = 1 */
    const float *lambda_char;
    void *out;                  /* [B, T, dim] */
    uint32_t *status;           /* optional, as in MotEmbedMixDesc */
    void *workspace;            /* mot_char_swa_workspace_bytes(desc) */
    size_t workspace_bytes;
    /* MOT_F32 (0) or MOT_BF16: where the two products over the tokens run (xq = wq xn, h = wo y).  MOT_BF16 = the bf16 MFMA with
     * fp32 accumulation, xn and y rounded to bf16 first and the weights taken as bf16 (for callers whose tables and weights
     * hold bf16 values; the reference script runs in float32), and the projected queries, keys and values kept as the bf16 tensors
     * they are in a bf16 cast of the module (fp32 softmax and sums); needs dim % 8 == 0 and (heads * head_dim) % 8 == 0. */
    int32_t matmul_dtype;
    /* 1 = `kv_tables` already holds this call's per-character key / value tables (skip building them) */
    int32_t kv_tables_ready;
    /* optional: caller-kept buffer of 2 * char_rows * n_heads * head_dim floats for the projected key / value rows of the character
     * table.  They depend on char_table, char_norm_w, wk and wv only, so an inference loop (what the reference file is) builds them
     * once: pass the buffer with kv_tables_ready = 0 after those change (the call fills it), = 1 otherwise. */
    void *kv_tables;
    /* MOT_F32 (0) or, with matmul_dtype == MOT_BF16, MOT_BF16: the element type of `out`.  bf16 is what the module returns in a bf16
     * cast: the last product then adds the fp32 residuals and writes bf16 itself (one rounding, as a caller's cast of the fp32 result
     * would do; a pass over [B, T, dim] less on each side of the boundary). */
    int32_t io_dtype;
    int32_t reserved1;   /* must be 0 */
} MotCharSwaDesc;

size_t mot_char_swa_desc_size(void);
size_t mot_char_swa_workspace_bytes(const MotCharSwaDesc *desc /* host */);
int mot_char_swa_fwd(const MotCharSwaDesc *desc /* host */, mot_stream_t stream);

/*
 * One decode step of the character mixer: row t of what mot_char_swa_fwd computes for a sequence, from the newest token alone and a
 * device-side state, for n_rows <= 16 sequences at once (the generation loop of inference/inference.py:411-489 with a KV cache in
 * the trunk needs only the newest row).  Rotary cancels (mot_swa.hip), so row t depends on the token at t, on the character ids of
 * the tokens t-window+1 .. t and on how many of those lie in front of the row's start.
 *   state   ring [n_rows, window, c_v] int32: the characters of source position s sit in slot s % window;
 *           pos  [n_rows] int64: the tokens of the row seen so far.
 *   call    t = pos[b]; the new token's characters (row tokens[b] of tok_chars, or char_ids_new[b]) go to slot t % window; the query
 *           attends over the window (a slot whose source position is < 0 is a padding key: score 0, a place in the softmax, zero
 *           value, as in mot_char_swa_fwd); pos[b] = t + 1.
 * `kv_tables` are the fp32 key / value tables that mot_char_swa_fwd fills (the prefill call): the step never builds them.
 * Three launches on `stream`; no allocation, sync, memset or memcpy node; nothing is read on the host, `tokens` is device memory
 * (mot_next_token's `token` is read in place).  Every sum has a fixed order: the same bits on every run.
 * dtype MOT_F32: fp32 tables and weights.  MOT_BF16: tok_table, char_table, wq and wo are bf16 and read in place, `out` is bf16;
 * the rounding points are those of mot_char_swa_fwd with matmul_dtype = io_dtype = MOT_BF16 (xn, q, k, v, y and the output of wo
 * are bf16 tensors; softmax and sums in fp32; the residuals are added to the bf16 output of wo in fp32, one rounding).
 * A token outside [0, tok_rows) raises MOT_STATUS_TOKEN_OOR and is treated as row 0 (mot_next_token's -1 included); a character id
 * outside [0, char_rows) raises MOT_STATUS_BYTE_OOR and is treated as id 0.
 */
typedef struct MotCharSwaStepDesc {
    uint32_t struct_size;         /* sizeof(MotCharSwaStepDesc) */
    int32_t dtype;                /* MOT_F32 or MOT_BF16 */
    int32_t n_rows;               /* B, 1 .. 16 (more: MOT_EUNSUPPORTED, use mot_char_swa_fwd) */
    int32_t c_v;                  /* characters per token */
    int32_t window;               /* window * c_v <= 64 */
    int32_t n_heads;
    int32_t head_dim;             /* 64 or 128 */
    int32_t dim;                  /* multiple of 4 (8 in bf16) */
    int32_t version;              /* MotSwaVersion */
    int32_t char_rows;
    const int64_t *tokens;        /* [n_rows] device */
    const int32_t *tok_chars;     /* [tok_rows, c_v] token -> character ids, or NULL */
    const int64_t *char_ids_new;  /* [n_rows, c_v] the new tokens' character ids, or NULL: exactly one of the two */
    const void *tok_table;        /* [tok_rows, dim] */
    int64_t tok_rows;
    const void *char_table;       /* [char_rows, dim] */
    const float *attn_norm_w;     /* [dim] fp32 in both modes */
    const void *wq;               /* [n_heads * head_dim, dim] */
    const void *wo;               /* [dim, n_heads * head_dim] */
    const float *lambda_tok;      /* fp32 device scalars (two_residual); NULL = 1 */
    const float *lambda_char;
    const float *kv_tables;       /* [2, char_rows, n_heads * head_dim] fp32, as mot_char_swa_fwd left them; required */
    int32_t *ring;                /* [n_rows, window, c_v] state, updated */
    int64_t *pos;                 /* [n_rows] state, updated */
    void *out;                    /* [n_rows, dim] */
    uint32_t *status;             /* optional */
    void *workspace;              /* mot_char_swa_step_workspace_bytes(desc) */
    size_t workspace_bytes;
    float norm_eps;               /* <= 0 -> 1e-5 */
    int32_t reserved0;            /* must be 0 */
    int64_t reserved1;            /* must be 0 */
} MotCharSwaStepDesc;

size_t mot_char_swa_step_desc_size(void);
size_t mot_char_swa_step_workspace_bytes(const MotCharSwaStepDesc *desc /* host */);   /* 0 for a descriptor the call would refuse */
int mot_char_swa_step(const MotCharSwaStepDesc *desc /* host */, mot_stream_t stream);

/*
 * The feed-forward that closes the character mixer's block, on the rows of a decode step (inference/inference.py:269, 121-144):
 *   out[r] = h[r] + w2 (silu(w1 xn[r]) * w3 xn[r]),   xn[r] = (h[r] * rs) * norm_w,  rs = 1 / sqrt(mean(h[r]^2) + norm_eps)
 * for n_rows <= 16 rows, h = the output of mot_char_swa_step.  Three launches on `stream` (gate-up: both of w1 and w3 in one pass
 * over the rows staged in LDS; down: w2 against slices of 1024 elements of inter, one workgroup per 16 columns and slice; the sum
 * of the slices' shares in slice order plus the residual); no allocation, sync, memset or memcpy node; nothing is read on the host;
 * no atomics.  Every sum has a fixed order that does not depend on n_rows: the same bits on every run, and for a row whatever rows
 * stand beside it.  silu(a) = a / (1 + exp(-a)) is finite for every finite a.
 * dtype MOT_F32: everything fp32.  MOT_BF16: h, w1, w2, w3 and out are bf16 and read in place (norm_w stays fp32); xn, a = w1 xn,
 * silu(a), b = w3 xn, silu(a) * b and the output of w2 are rounded to bf16, all sums are fp32, the residual is added to the widened
 * output of w2 in fp32 and rounded once.
 * Refused before any HIP call, by the size query too (it then returns 0): a wrong struct_size, an unknown dtype, non-zero reserved
 * fields (MOT_EINVAL); n_rows outside 1..16 (MOT_EUNSUPPORTED: use the torch path); dim or inter not a multiple of 4, inter above
 * 2^24 (MOT_ESHAPE), not a multiple of 8 in bf16 (MOT_EUNSUPPORTED) -- the slices need nothing more, the last one may be short;
 * staged rows R * dim * sizeof(element) above 128 KiB, R = n_rows rounded up to 1, 2, 4, 8 or 16 (MOT_EUNSUPPORTED); a NULL h,
 * norm_w, w1, w3, w2 or out (MOT_EINVAL); one of them not 16-byte aligned (MOT_EUNSUPPORTED); out overlapping h (MOT_EINVAL).
 * Workspace: align256(n_rows * inter * sizeof(element)) + align256(ceil(inter / 1024) * n_rows * dim * 4) bytes.
 */
typedef struct MotFfnStepDesc {
    uint32_t struct_size;         /* sizeof(MotFfnStepDesc) */
    int32_t dtype;                /* MOT_F32 or MOT_BF16 */
    int32_t n_rows;               /* 1 .. 16 */
    int32_t dim;                  /* multiple of 4 (8 in bf16) */
    int32_t inter;                /* multiple of 4 (8 in bf16) */
    int32_t reserved0;            /* must be 0 */
    const void *h;                /* [n_rows, dim] */
    const float *norm_w;          /* [dim] fp32 in both modes */
    const void *w1;               /* [inter, dim] */
    const void *w3;               /* [inter, dim] */
    const void *w2;               /* [dim, inter] */
    void *out;                    /* [n_rows, dim]; must not overlap h */
    uint32_t *status;             /* optional; reserved, the call raises no flag */
    void *workspace;              /* mot_ffn_step_workspace_bytes(desc) */
    size_t workspace_bytes;
    float norm_eps;               /* <= 0 -> 1e-5 */
    int32_t reserved1;            /* must be 0 */
    int64_t reserved2;            /* must be 0 */
} MotFfnStepDesc;

size_t mot_ffn_step_desc_size(void);
size_t mot_ffn_step_workspace_bytes(const MotFfnStepDesc *desc /* host */);   /* 0 for a descriptor the call would refuse */
int mot_ffn_step(const MotFfnStepDesc *desc /* host */, mot_stream_t stream);

/*
 * Byte output head of a mixout run with identity ByteSelfAttn layers (use_byte_self_attn off), forward: replaces
 *   ByteMixoutCopy / ByteMixoutSplit.forward          scaled-pre-train/train_gpt.py:483-527 (ByteSelfAttn identity, 382-419)
 *   and the head of GPT.forward                       :618-623  (x = byte_mixout(x); norm; lm_head; 30 sigmoid(l / 7.5); cross_entropy)
 * Rows: copy = the token rows of x [n_tokens, model_dim] (every byte row of a token is the same row); split = the byte rows of x
 * viewed as [n_tokens * bpt, model_dim / bpt].  Per row, h <- h + norm(h) n_layer_out times, then l = norm(h) W^T, z = 30 sigmoid(l / 7.5);
 * the loss is the mean over all M = n_tokens * bpt targets of lse(z) - z[y] (no ignore_index), written as one fp32 scalar; the sum runs
 * in a fixed order, so the same inputs give the same bits.  A target outside [0, vocab) addresses nothing: its term leaves the sum
 * (the mean still divides by M) and MOT_STATUS_TARGET_OOR is ORed into `status`.
 * dtype follows x: MOT_F32, or MOT_BF16 with `weight` already cast to bf16 (CastedLinear, train_gpt.py:185-186): the products run on
 * the bf16 MFMA with fp32 accumulation, the epilogue and the loss in fp32.  vocab must be 512 (next_multiple_of_n(458, n=128), :574);
 * the row width K (model_dim, or model_dim / bpt in split mode) a multiple of 16 and at most 2048.  Checked before any HIP call:
 * an unknown method, dtype, vocab or row width returns MOT_EUNSUPPORTED, a shape the reference asserts on MOT_ESHAPE.
 */
typedef enum MotByteHeadMethod { MOT_HEAD_COPY = 0, MOT_HEAD_SPLIT = 1 } MotByteHeadMethod;

typedef struct MotByteHeadDesc {
    uint32_t struct_size; /* sizeof(MotByteHeadDesc) */
    int32_t method;       /* MotByteHeadMethod */
    int32_t dtype;        /* MotDType of x and weight */
    int32_t bpt;          /* bytes per token */
    int64_t n_tokens;     /* B * T */
    int32_t model_dim;    /* columns of x */
    int32_t n_layer_out;  /* identity mixout layers, h <- h + norm(h) */
    int32_t vocab;        /* rows of weight: 512 */
    float eps;            /* of every norm; <= 0 -> FLT_EPSILON: F.rms_norm(eps=None) takes the epsilon of its fp32 opmath type,
                             on bf16 inputs too (checked against the reference's bf16 outputs) */
    const void *x;        /* [n_tokens, model_dim], 16-byte aligned */
    const void *weight;   /* [vocab, K] lm_head.weight in dtype, 16-byte aligned */
    const int64_t *targets; /* [n_tokens * bpt] byte targets, token-major */
    float *loss;          /* forward: fp32 scalar */
    float *row_stats;     /* [2 * rows] fp32: the forward writes lse of every row, then its norm factor c; the backward reads them */
    uint32_t *status;     /* optional, as in MotEmbedMixDesc */
    void *workspace;      /* >= mot_byte_head_workspace_bytes(desc), for the forward and the backward */
    size_t workspace_bytes;
} MotByteHeadDesc;

size_t mot_byte_head_desc_size(void);
size_t mot_byte_head_workspace_bytes(const MotByteHeadDesc *desc /* host */);
int mot_byte_head_fwd(const MotByteHeadDesc *desc /* host */, mot_stream_t stream);
/*
 * Backward (loss.backward(), train_gpt.py:1319): `desc` as in the forward, with the row_stats it wrote.  grad_loss is a device fp32
 * scalar (never read on the host, so the pair is hipGraph-capturable).  dx [n_tokens, model_dim] in dtype and dW [vocab, K] fp32 are
 * OVERWRITTEN.  dx is written once per row (the same bits every run); dW sums products over the rows with fp32 atomics.
 */
int mot_byte_head_bwd(const MotByteHeadDesc *desc /* host */, const float *grad_loss, void *dx, float *dW, mot_stream_t stream);

/*
 * The split-mode training step in ONE call: mot_byte_head_fwd followed by mot_byte_head_bwd with grad_loss = 1 (the caller scales dx
 * and dW by the incoming gradient on the device, as with mot_token_head_fwd), on one fused kernel: each workgroup of a persistent
 * grid holds W in LDS and walks tiles of 256 byte rows; a tile's logits are formed on the MFMA with the rows on the lanes, and the
 * cap, the loss term, G, u = G W and the row chain stay in registers, so nothing 512 wide per row goes to memory on the way to loss
 * and dx.  dW = G^T x: the kernel stores a chunk's G in dtype (bf16: 1 KB a row; 131 072 rows a chunk) and the shared product adds
 * the chunk into dW with fp32 atomics, as mot_byte_head_bwd does.
 *   loss   as mot_byte_head_fwd: fixed-order sum, the same bits every run; out-of-range targets as there (term dropped, G row zero,
 *          so that row of dx is exactly zero, M stays, MOT_STATUS_TARGET_OOR raised).
 *   dx     [n_tokens, model_dim] in dtype, written once per element, the same bits every run; the row chain is mot_byte_head_bwd's.
 *   dW     [512, K] fp32, OVERWRITTEN (the caller zeroes nothing).
 *   dx = dW = NULL: the loss alone, nothing written per logit, the same loss bits.  One of the two NULL: MOT_EINVAL.
 * desc->row_stats is ignored (may be NULL); eps <= 0 as above.  Asynchronous on `stream`, no allocation, no host read, no memset or
 * memcpy node: hipGraph-capturable.  bf16 rounding points are those of the pair: G rounded once to bf16, u in fp32, dx rounded once.
 * Built: method MOT_HEAD_SPLIT, vocab 512, K = model_dim / bpt a multiple of 16 and at most 128 in MOT_BF16, 64 in MOT_F32 (W and
 * its staging must fit in LDS).  Everything else is refused before any HIP call, mot_last_error() starting with "byte_head_step":
 * MOT_EUNSUPPORTED for copy mode (use mot_byte_head_fwd / _bwd), another vocab, an unknown dtype, K not a multiple of 16 or above
 * its bound, n_tokens * bpt > 2^31, a misaligned x, weight or dx; MOT_ESHAPE for the shapes mot_byte_head_fwd refuses and for no
 * targets; MOT_EINVAL for a null x, weight, targets or loss; MOT_EWORKSPACE (with the size) for a missing or short workspace.
 * The workspace query returns 0 for a refused descriptor.
 */
size_t mot_byte_head_step_workspace_bytes(const MotByteHeadDesc *desc /* host */);
int mot_byte_head_step(const MotByteHeadDesc *desc /* host */, void *dx, float *dW, mot_stream_t stream);

/*
 * Token-level output head, forward and backward in one call: replaces the last five lines of every training script
 *   scaled-pre-train/train_gpt.py:619-623 with byte_mixout_method "noop"   (norm; lm_head; 30 sigmoid(l.float() / 7.5); cross_entropy)
 *   modded-nanogpt/runs/71_*.py:331-334, and the other 49 runs alike       (norm; F.linear; 15 l rsqrt(l^2 + 225); cross_entropy)
 * Per row r of x [n_rows, model_dim], weight [vocab, model_dim], targets [n_rows]:
 *   c_r = (mean(x_r^2) + eps)^-1/2 with norm_in, else 1;   l = c_r (x_r W^T);   z = cap(l)  (MotSoftcap);
 *   loss = (1 / n_rows) sum_r (lse(z_r) - z_r[y_r]), one fp32 scalar from a fixed-order sum: the same inputs give the same bits.
 * There is no ignore_index (the reference passes none): a target outside [0, vocab), -100 included, addresses nothing.  Its term
 * leaves the sum, its rows of the gradients are exactly zero, the mean still divides by n_rows, and MOT_STATUS_TARGET_OOR is ORed
 * into `status`.  Rows 50 257 .. 50 303 of a 50 304-row weight are ordinary classes.
 * With dx and dW NULL the call is the loss alone (eval, no_grad): one product per chunk, nothing written per logit.  With either set,
 * the same pass over a chunk also forms the gradients FOR grad_loss = 1 (the caller scales them by the incoming gradient):
 *   dx [n_rows, model_dim] in dtype, written once per row (the same bits every run);
 *   dW [vocab, model_dim] fp32, zeroed by the call, then summed over the rows with fp32 atomics.
 * So a chunk's logits are formed once, and a training step costs three products of 2 n_rows vocab model_dim FLOP.  No buffer of
 * n_rows x vocab exists: the rows run in chunks of `chunk_rows`, and the workspace holds the logits of one chunk (fp32; bf16 in
 * MOT_BF16, where the reference's lm_head returns bf16 too), and, when dx is set, the chunk's u = G W (fp32) and in MOT_BF16 a
 * transposed copy of the weight.  chunk_rows = 0 is the library's choice: the largest multiple of 256 rows whose logits and u stay
 * below 512 MiB (2560 rows of fp32 logits, 5120 of bf16, at 50 304 x 768), at least 256; a chunk never exceeds n_rows.
 * dtype follows x: MOT_F32, or MOT_BF16 with `weight` already cast to bf16 (products on the bf16 MFMA with fp32 accumulation, the
 * row pass in fp32).  Checked before any HIP call, with a message: vocab not a multiple of 128 or above 262 144, model_dim not a
 * multiple of 16 or above 2048, an unknown dtype or softcap -> MOT_EUNSUPPORTED; chunk_rows neither 0 nor a multiple of 32 ->
 * MOT_ESHAPE; chunk_rows x vocab above 2^31 -> MOT_EUNSUPPORTED.  The workspace query returns 0 for a descriptor the call refuses;
 * it reads dx (set or NULL) and no other pointer.
 */
typedef enum MotSoftcap {
    MOT_SOFTCAP_SIGMOID30 = 0, /* z = 30 sigmoid(l / 7.5), 0 < z < 30    (train_gpt.py:622)      */
    MOT_SOFTCAP_RSQRT15 = 1    /* z = 15 l (l^2 + 225)^-1/2, |z| < 15    (runs/71_*.py:334)      */
} MotSoftcap;

typedef struct MotTokenHeadDesc {
    uint32_t struct_size; /* sizeof(MotTokenHeadDesc) */
    int32_t dtype;        /* MotDType of x, weight and dx */
    int32_t softcap;      /* MotSoftcap */
    int32_t norm_in;      /* 1: x is rms-normed first (line 619 / 331), 0: x is taken as it is */
    int64_t n_rows;       /* B * T */
    int32_t model_dim;    /* columns of x and of weight */
    int32_t vocab;        /* rows of weight: 50 304 = next_multiple_of_n(50257, n=128) */
    float eps;            /* of the norm; <= 0 -> FLT_EPSILON, as F.rms_norm(eps=None) takes it, on bf16 inputs too */
    int32_t chunk_rows;   /* rows per chunk: 0 = the library's choice, else a multiple of 32 */
    const void *x;        /* [n_rows, model_dim], 16-byte aligned */
    const void *weight;   /* [vocab, model_dim] in dtype, 16-byte aligned */
    const int64_t *targets; /* [n_rows] */
    float *loss;          /* fp32 scalar */
    float *row_stats;     /* optional [2 * n_rows] fp32: lse(z_r) of every row, then its norm factor c_r */
    uint32_t *status;     /* optional, as in MotEmbedMixDesc */
    void *workspace;      /* >= mot_token_head_workspace_bytes(desc), 16-byte aligned */
    size_t workspace_bytes;
    void *dx;             /* optional [n_rows, model_dim] in dtype, 16-byte aligned, OVERWRITTEN */
    float *dW;            /* optional [vocab, model_dim] fp32, 16-byte aligned, OVERWRITTEN */
} MotTokenHeadDesc;

size_t mot_token_head_desc_size(void);
size_t mot_token_head_workspace_bytes(const MotTokenHeadDesc *desc /* host */);
int mot_token_head_fwd(const MotTokenHeadDesc *desc /* host */, mot_stream_t stream);

/*
 * Evaluation form of the two output heads: the pass of the loss call without gradients over the same chunks, which also writes
 * what it knows about every row.  A row is a token for the token-level head and a byte position for the byte head (n_tokens * bpt
 * of them, token-major, as `targets` are; in copy mode the head still computes one row per token and writes it out per position).
 * `desc` is the descriptor of the loss call: desc->loss receives the same fixed-order sum with the same bits as mot_token_head_fwd
 * with dx = dW = NULL / mot_byte_head_fwd on the same inputs.  No gradients are formed and nothing of rows x vocab exists.
 *   row_loss[r] = lse(z_r) - z_r[y_r] in fp32: the term the loss sums.
 *   pred[r]     = the class with the largest logit, taken on the chunk's stored product s = x W^T (fp32; bf16 in the token-level
 *                 head's MOT_BF16 mode, compared as stored) in front of the row factor c_r > 0 and the strictly increasing softcap:
 *                 the argmax of z_r, an exact function of what the product stored.  Ties go to the lowest class index; the padded
 *                 classes (50 257 .. 50 303, 458 .. 511) are ordinary classes, as in the loss.
 *   rank[r]     = the number of classes whose stored s is strictly greater than the target's: 0 = the target is (one of) the
 *                 largest; rank < k is top-k accuracy, 1 / (1 + rank) the reciprocal rank.
 *   counts      = int64 [n_rows_counted, n_top1] on the device: the rows with a target inside [0, vocab), and those of them with
 *                 pred == target.  mot_byte_head_eval writes a third: n_tokens_all_correct, the tokens whose bpt byte predictions
 *                 all equal their targets.  Integer sums: the same on every run.  Never read on the host: the call is capturable.
 * A target outside [0, vocab) is handled as in the loss call (its term leaves the sum, MOT_STATUS_TARGET_OOR is raised), and here
 * row_loss = 0, rank = -1, pred is still written, the row is left out of both counts and its token cannot be all-correct.
 * Each output pointer may be NULL, except that `counts` is closed from `pred` and the targets, so counts needs pred.  Every output
 * is written once per row with plain stores.  row_loss, pred and rank must be 4-byte aligned, counts 8-byte aligned.
 * Workspace: that of the loss call without gradients, i.e. mot_token_head_workspace_bytes(desc) with desc->dx == NULL (the query
 * reads no other pointer) and mot_byte_head_workspace_bytes(desc).  desc->row_stats is optional in both calls.
 * Checked before any HIP call, with a message that starts with the function's name: a null descriptor or out struct, a wrong
 * struct_size, reserved != 0, a misaligned pointer, counts without pred, dx or dW set in the token descriptor (the call forms no
 * gradients) -> MOT_EINVAL; every shape and dtype refusal of the loss call, with its codes.
 */
typedef struct MotHeadEvalOut {
    uint32_t struct_size; /* sizeof(MotHeadEvalOut) */
    uint32_t reserved;    /* 0 */
    float *row_loss;      /* optional [rows] fp32 */
    int32_t *pred;        /* optional [rows] */
    int32_t *rank;        /* optional [rows] */
    int64_t *counts;      /* optional [2] (token-level head) or [3] (byte head); needs pred */
} MotHeadEvalOut;

size_t mot_head_eval_out_size(void);
int mot_token_head_eval(const MotTokenHeadDesc *desc /* host */, const MotHeadEvalOut *out /* host */, mot_stream_t stream);
int mot_byte_head_eval(const MotByteHeadDesc *desc /* host */, const MotHeadEvalOut *out /* host */, mot_stream_t stream);

/*
 * Plain cross-entropy head, forward and backward in one call: lm_head and F.cross_entropy on the logits as they are, with NO softcap,
 * with ignore_index, and with the mean taken over the kept targets.  Replaces the loss of the reference's two remaining loops:
 *   mathblations/model.py:337-338 with main.py:294-303, evaluation main.py:164-187
 *       (F.rms_norm(x); lm_head(x).float(); slice_logits_and_targets; F.cross_entropy; argmax accuracies; 50 304 classes in fp32)
 *   inference/inference.py:349-359
 *       (lm_head(hidden_states); shift; CrossEntropyLoss(), i.e. ignore_index -100 and the mean over the kept targets; 128 256
 *        classes at model_dim 2048, hidden states already normed: norm_in = 0, the shift stays with the caller)
 * mot_token_head_* cannot serve them: its row pass takes lse from the softcap's constant bound, it has no ignore_index and it
 * divides by n_rows.  Per row r of x [n_rows, model_dim], weight [vocab, model_dim], targets [n_rows]:
 *   c_r = (mean(x_r^2) + eps)^-1/2 with norm_in, else 1;   l = c_r (x_r W^T);   m_r = max_v l;   lse_r = m_r + log sum_v exp(l - m_r).
 * The product is stored per chunk in fp32, or in bf16 in MOT_BF16 (where lm_head returns bf16); everything behind it is fp32:
 * cross_entropy(lm_head(x).float(), y), the expression of model.py:338.
 * A row is KEPT when 0 <= y_r < vocab and y_r != ignore_index; `kept` is the number of kept rows.  A target equal to ignore_index
 * drops its row silently (set the field to -100 for torch's default, or to any value no target takes); any other target outside
 * [0, vocab) drops its row too and ORs MOT_STATUS_TARGET_OOR into `status` (torch would assert there).
 *   loss = (sum over kept rows of (lse_r - l_r[y_r])) / kept: one fp32 scalar from the heads' fixed-order double sum, the same bits
 *          on every run.  kept == 0 gives NaN (0 / 0, as F.cross_entropy returns) and gradients that are exactly zero.
 * Scoring the window [start, end) of each sequence (slice_logits_and_targets) is this loss with every other position's target set
 * to ignore_index.  `kept` is counted on the device in front of the first chunk and never read on the host: no allocation, no host
 * read, no memset or memcpy node, so loss, dx and dW capture into a hipGraph, and a replay follows targets changed in place.
 * With dx and dW NULL the call is the loss alone.  With either set the same pass over a chunk forms the gradients FOR grad_loss = 1:
 *   G_r = (c_r / kept) (softmax(l_r) - onehot(y_r)) for a kept row, a row of zeros otherwise;   u = G W;
 *   dx [n_rows, model_dim] in dtype = u_r - c_r^2 (x_r . u_r / model_dim) x_r with norm_in, else u_r; written once per row;
 *   dW [vocab, model_dim] fp32 = G^T x, zeroed by the call, then summed over the rows with fp32 atomics.
 * Chunks, workspace and shapes are the token-level head's: chunk_rows = 0 is the largest multiple of 256 rows whose logits and u
 * stay below 512 MiB (2560 rows of fp32 logits at 50 304 x 768; 1024 of fp32 and 1792 of bf16 logits at 128 256 x 2048), at least
 * 256, never more than n_rows.  Checked before any HIP call, with a message that starts with the function's name: vocab not a
 * multiple of 128 or above 262 144, model_dim not a multiple of 16 or above 2048, an unknown dtype -> MOT_EUNSUPPORTED; chunk_rows
 * neither 0 nor a multiple of 32, group_rows negative or not dividing n_rows, no rows -> MOT_ESHAPE; chunk_rows x vocab above 2^31
 * -> MOT_EUNSUPPORTED; a null descriptor, x, weight, targets or loss, a wrong struct_size -> MOT_EINVAL; a missing or short workspace
 * -> MOT_EWORKSPACE; a misaligned pointer -> MOT_EUNSUPPORTED.  The workspace query returns 0 for what the call refuses; it reads
 * dx (set or NULL) and no other pointer.
 * mot_plain_head_eval is the evaluation form (MotHeadEvalOut above, dx = dW = NULL): row_loss, pred and rank as defined there on the
 * stored product (c_r > 0 changes no order), the lowest class on ties; for a dropped row row_loss = 0, rank = -1, pred still
 * written.  desc->loss has the bits of mot_plain_head_fwd without gradients.  counts = int64 [kept, kept rows with pred == target],
 * and with group_rows > 0 a third entry: the groups of group_rows consecutive rows (a sequence) that have at least one kept row and
 * whose kept rows are ALL right, full_correct of main.py:183-187.  Dropped rows count neither for nor against their group (the byte
 * head's third count differs there).  group_rows is read by the evaluation alone.
 * These two calls form the logits of every row, kept or not; mot_plain_head_compact_* below form them for the kept rows alone.
 * Not built: label smoothing; the 14-class digit head of digit_mixout_method != "noop".
 */
typedef struct MotPlainHeadDesc {
    uint32_t struct_size; /* sizeof(MotPlainHeadDesc) */
    int32_t dtype;        /* MotDType of x, weight and dx */
    int32_t norm_in;      /* 1: x is rms-normed first (model.py:337), 0: x is taken as it is (inference.py:349) */
    int32_t chunk_rows;   /* rows per chunk: 0 = the library's choice, else a multiple of 32 */
    int64_t n_rows;       /* B * T */
    int32_t model_dim;    /* columns of x and of weight */
    int32_t vocab;        /* rows of weight: 50 304, 128 256 */
    float eps;            /* of the norm; <= 0 -> FLT_EPSILON, as F.rms_norm(eps=None) takes it, on bf16 inputs too */
    int32_t group_rows;   /* evaluation: rows per group (a sequence) of the third count; 0 = two counts */
    int64_t ignore_index; /* targets equal to it drop their rows silently; torch's default is -100 */
    const void *x;        /* [n_rows, model_dim], 16-byte aligned */
    const void *weight;   /* [vocab, model_dim] in dtype, 16-byte aligned */
    const int64_t *targets; /* [n_rows] */
    float *loss;          /* fp32 scalar */
    uint32_t *status;     /* optional, as in MotEmbedMixDesc */
    void *workspace;      /* >= mot_plain_head_workspace_bytes(desc), 16-byte aligned */
    size_t workspace_bytes;
    void *dx;             /* optional [n_rows, model_dim] in dtype, 16-byte aligned, OVERWRITTEN */
    float *dW;            /* optional [vocab, model_dim] fp32, 16-byte aligned, OVERWRITTEN */
} MotPlainHeadDesc;

size_t mot_plain_head_desc_size(void);
size_t mot_plain_head_workspace_bytes(const MotPlainHeadDesc *desc /* host */);
int mot_plain_head_fwd(const MotPlainHeadDesc *desc /* host */, mot_stream_t stream);
int mot_plain_head_eval(const MotPlainHeadDesc *desc /* host */, const MotHeadEvalOut *out /* host */, mot_stream_t stream);

/*
 * The plain head with the kept rows compacted in front of the products: the time follows the number of scored positions, not
 * n_rows.  `desc` and everything stated above hold (kept rows, `kept`, loss, G, dx, dW, MOT_STATUS_TARGET_OOR, NaN at kept == 0,
 * dtypes, shape limits); the count of kept rows still lives on the device alone, so the caller passes a bound it knows on the host
 * (the window lengths, the label mask's shape): max_kept.
 *   cap = min(max_kept, n_rows).  The kept rows are taken in ascending row order into slots 0 .. kept-1 by an index pass over the
 *   targets (per-workgroup counts, a scan of the counts, per-workgroup writes: three launches, no workgroup waits on another).
 *   Slots kept .. cap-1 are padding: zero rows with an ignored target, which add nothing to the loss, have G = 0 and add exactly
 *   nothing to dW.  Per chunk the slots' rows of x and their targets are gathered, the products and the row pass run per slot,
 *   and the row chain writes each valid slot's gradient straight into its row of dx.
 *   With norm_in the norm is applied in the gather: the slot's row is h = c_r x_r, rounded to dtype as F.rms_norm's output is in
 *   front of lm_head, and l = h W^T is stored per chunk as above.  The same l, G, dx and dW mathematically; in MOT_BF16 the
 *   logits carry the reference's own two roundings (norm(x), then the product), where mot_plain_head_fwd scales the stored
 *   product of the un-normed row in fp32.  pred and rank of the evaluation are taken on the stored h W^T.
 *   The chunk rule runs over cap: chunk_rows = 0 is the rule above with cap in place of n_rows, a given chunk_rows is clipped to
 *   cap.  The number of chunks, every grid and the workspace depend on host values only, so whole padding chunks still run their
 *   products on zero rows: a tight bound is the caller's job.
 *   loss: the fixed-order double sum over the slots' terms divided by the device count; the same bits on every run, NOT necessarily
 *   those of mot_plain_head_fwd (the sum is grouped differently and a chunk of another height may take another product route).
 *   dx [n_rows, model_dim]: every element is written by the call, a kept row's gradient once, +0 in every element of a dropped row
 *   (by a kernel, no memset node).  dW = G^T x over the gathered rows, zeroed by the call, summed with fp32 atomics as above.
 *   kept > cap is a caller error: MOT_STATUS_KEPT_OVERFLOW is ORed into `status` and the call behaves as if nothing were kept
 *   (loss NaN, dx and dW exactly zero); it never scores only the first cap rows.
 * mot_plain_head_compact_eval: row_loss, pred and rank stay per original row.  A kept row gets what mot_plain_head_eval writes; a
 * dropped row gets row_loss = 0, rank = -1 and pred = -1 (its logits are never formed: the one difference from mot_plain_head_eval,
 * which still writes a dropped row's pred).  counts as above, group_rows included.  desc->loss has the bits of
 * mot_plain_head_compact_fwd without gradients.
 * No allocation, no host read, no memset or memcpy node: the calls capture into a hipGraph, and a replay follows targets changed in
 * place, a change of kept in either direction and into and out of overflow included.
 * Checked before any HIP call, with a message that starts with the function's name: everything the calls above refuse, with the same
 * codes; a null or wrongly sized MotPlainHeadCompact or reserved != 0 -> MOT_EINVAL; max_kept <= 0 -> MOT_ESHAPE.  max_kept > n_rows
 * is clipped.  The workspace query returns 0 for what the calls refuse; it is at least mot_plain_head_workspace_bytes(desc) at
 * max_kept >= n_rows and shrinks with max_kept.
 */
typedef struct MotPlainHeadCompact {
    uint32_t struct_size; /* sizeof(MotPlainHeadCompact) */
    uint32_t reserved;    /* 0 */
    int64_t max_kept;     /* host bound on the number of kept rows; > 0; clipped to n_rows */
} MotPlainHeadCompact;

size_t mot_plain_head_compact_size(void);
size_t mot_plain_head_compact_workspace_bytes(const MotPlainHeadDesc *desc /* host */, const MotPlainHeadCompact *compact /* host */);
int mot_plain_head_compact_fwd(const MotPlainHeadDesc *desc /* host */, const MotPlainHeadCompact *compact /* host */, mot_stream_t stream);
int mot_plain_head_compact_eval(const MotPlainHeadDesc *desc /* host */, const MotPlainHeadCompact *compact /* host */,
                                const MotHeadEvalOut *out /* host */, mot_stream_t stream);

/*
 * The generation step behind the plain head: the last position's logits, the top-k and top-p cuts and the draw in ONE call.
 * Replaces the loop body of inference/inference.py:420-444 (lm_head on the last position / temperature; torch.topk; a full
 * torch.sort of 128 256 logits with cumsum, scatter and softmax; argmax or multinomial; .item()) and the print of :448-453.
 * Shapes and conventions are the plain head's: vocab a multiple of 128 up to 262 144, model_dim a multiple of 16 up to 2048,
 * norm_in, bf16 logits as stored.  Per row r of x [n_rows, model_dim], rows x_stride ELEMENTS apart (hidden[:, -1, :] passes
 * without a copy; x_stride * sizeof(dtype) must be a multiple of 16):
 *  1. h = c x_r with c = (mean(x_r^2) + eps)^-1/2 (norm_in), else h = x_r; with norm_in h is rounded to dtype, as F.rms_norm's
 *     output is in front of lm_head.  l = h W^T is STORED in fp32, or in bf16 in MOT_BF16; everything behind it is fp32 or integer.
 *     `logits` (optional, fp32 [n_rows, vocab]) receives the stored values, widened, in front of the temperature.
 *  2. All order decisions are taken on the stored logits (-0 counts as +0); temperature > 0 keeps their order.  The mass of a class is
 *     exp((l - m) / temperature) with m the row's maximum, held as an integer number of 2^-44 rounded UP (at least one unit for a
 *     finite logit, none for -inf): every sum of masses is an integer sum, the same bits on every run and in every order.  The
 *     rounding adds at most vocab * 2^-44 (1.5e-8) to a total of at least 1.
 *  3. top-k (line 423-425) applies when 0 < top_k < vocab: a class stays when l >= the k-th largest value.  Ties with that value all
 *     stay, as the reference's `<` leaves them.
 *  4. top-p (line 428-437) applies when top_p < 1, over the survivors of 3 with their masses renormalised: a class stays when the mass
 *     of the STRICTLY LARGER logits is <= top_p.  For distinct logits that is the reference (its shift by one keeps the first class
 *     that crosses).  Among equal logits torch.sort promises no order, so the reference leaves open which members of a tie group on
 *     the boundary stay; this call keeps a tie group whole.  That is the one place where it pins what the reference leaves open.
 *  5. greedy: the largest logit, the lowest class on ties (the evaluation's rule).  Otherwise the inverse CDF over the kept classes
 *     in ascending class order with the caller's u[r]: the first kept class whose running mass exceeds u Z (Z: the kept mass).  u is
 *     clamped into [0, 1 - 2^-24], a NaN counts as 0; if rounding lets no class exceed u Z, the last kept class is returned: never
 *     an unkept class, never vocab.  The random number itself (torch.rand, capture-aware) stays with the caller, which makes the call
 *     reproducible.
 *  6. token int64 [n_rows]; prob (optional) the filtered probability of the returned token; kept (optional, int32) the number of
 *     surviving classes; top_cls / top_prob (optional, [n_rows, n_top], n_top <= 8) the largest filtered probabilities in descending
 *     order, the lowest class first on ties, -1 / 0 past the kept count.
 *  7. A row with a NaN or +inf logit (or with no finite logit at all) returns token = -1, prob = NaN, kept = 0, top_cls = -1,
 *     top_prob = 0 and ORs MOT_STATUS_LOGIT_NONFINITE into `status`; the other rows are unaffected.
 *  8. No allocation, no host read, no memset or memcpy node: the call captures into a hipGraph and a replay follows x, weight and u
 *     changed in place (temperature, top_k, top_p, greedy and n_top are host values of the captured call).
 *  9. n_rows = 0 is a no-op.  Up to 16 rows take a product kernel that reads W once; more rows take the heads' product in chunks whose
 *     logits stay below 512 MiB.
 * Checked before any HIP call, with a message that starts with the function's name: a null descriptor or a wrong struct_size ->
 * MOT_EINVAL; dtype, vocab, model_dim, a misaligned x_stride or pointer -> MOT_EUNSUPPORTED; n_rows < 0 or x_stride < model_dim ->
 * MOT_ESHAPE; temperature <= 0 or not finite, top_k < 0, top_p <= 0 or NaN, n_top outside 0..8, reserved != 0, a null u without
 * greedy, a null x, weight or token -> MOT_EINVAL; a missing or short workspace -> MOT_EWORKSPACE.  The workspace query returns 0 for
 * a descriptor the call would refuse (it ignores workspace and workspace_bytes) and for n_rows = 0.
 * Not built: the trunk and its KV cache, a random generator inside the kernel, repetition penalties, beam search, gradients.
 */
typedef struct MotNextTokenDesc {
    uint32_t struct_size; /* sizeof(MotNextTokenDesc) */
    int32_t dtype;        /* MotDType of x and weight */
    int32_t norm_in;      /* 1: x is rms-normed first, 0: x is taken as it is (inference.py: hidden states already normed) */
    int32_t greedy;       /* 1: the largest logit; 0: the draw with u */
    int64_t n_rows;       /* sequences in the batch */
    int64_t x_stride;     /* elements between rows of x, >= model_dim */
    int32_t model_dim;    /* columns of x and of weight */
    int32_t vocab;        /* rows of weight */
    float eps;            /* of the norm; <= 0 -> FLT_EPSILON */
    float temperature;    /* > 0 */
    int32_t top_k;        /* 0 or >= vocab: no cut */
    float top_p;          /* > 0; >= 1: no cut */
    int32_t n_top;        /* 0..8 columns of top_cls / top_prob */
    int32_t reserved;     /* 0 */
    const void *x;        /* [n_rows] rows of model_dim, 16-byte aligned */
    const void *weight;   /* [vocab, model_dim] in dtype, 16-byte aligned */
    const float *u;       /* [n_rows] uniform numbers of the caller; may be NULL with greedy */
    int64_t *token;       /* [n_rows] */
    float *prob;          /* optional [n_rows] */
    int32_t *kept;        /* optional [n_rows] */
    int32_t *top_cls;     /* optional [n_rows, n_top] */
    float *top_prob;      /* optional [n_rows, n_top] */
    float *logits;        /* optional [n_rows, vocab] fp32, 16-byte aligned */
    uint32_t *status;     /* optional, as in MotEmbedMixDesc */
    void *workspace;      /* >= mot_next_token_workspace_bytes(desc), 16-byte aligned */
    size_t workspace_bytes;
} MotNextTokenDesc;

size_t mot_next_token_desc_size(void);
size_t mot_next_token_workspace_bytes(const MotNextTokenDesc *desc /* host */);
int mot_next_token(const MotNextTokenDesc *desc /* host */, mot_stream_t stream);

/*
 * Byte self-attention in front of the concat mixin, forward: replaces ByteSelfAttn.forward with use_byte_self_attn on
 *   scaled-pre-train/train_gpt.py:382-418 around CausalSelfAttention.forward :226-240 (Rotary 189-206, norm 172-173)
 * x [n_rows, row_len, dim] are the byte embeddings of n_rows batch rows, row_len = T * bpt byte positions each.
 *   (q, k, v) = x qkv_w^T per head of 128 columns; q, k <- rms_norm over the head, then rotary with the byte's index in its batch
 *   row; v <- lambda_v v; p = softmax(0.12 q.k) over the allowed keys; out = x + (sum p v) proj_w^T.
 * Key j is allowed for query i of the same batch row when i - j < window and j <= i (block_causal = 0) or
 * j / bpt <= i / bpt (block_causal = 1).  window is in bytes (sliding_window_tokens * bpt), at most 256.
 * fp32 only; bf16 tensors are the follow-up and return MOT_EUNSUPPORTED.  Asynchronous on `stream`, no host synchronisation.
 * The forward leaves the raw projections, the attention output and the row statistics in `saved`
 * (mot_byte_self_attn_saved_bytes: 2052 * n_heads bytes per byte position) for the backward; it needs no workspace, the backward does.
 */
typedef struct MotByteSelfAttnDesc {
    uint32_t struct_size;   /* sizeof(MotByteSelfAttnDesc) */
    int32_t dtype;          /* MOT_F32 */
    int64_t n_rows;         /* B */
    int64_t row_len;        /* L = T * bpt byte positions per batch row */
    int32_t bpt;            /* bytes per token */
    int32_t window;         /* bytes: 1 .. 256, a multiple of bpt */
    int32_t block_causal;   /* mix_byte_in_tok */
    int32_t dim;            /* columns of x: a multiple of 16, at most 2048 */
    int32_t n_heads;        /* max(1, dim / 128) */
    int32_t head_dim;       /* 128 */
    const void *x;          /* [n_rows * row_len, dim] */
    const void *qkv_w;      /* [3, n_heads * 128, dim] */
    const void *proj_w;     /* [dim, n_heads * 128] c_proj.weight */
    const float *lambda_v;  /* device scalar: lambdas[0] */
    const float *cos, *sin; /* [rope_rows, 64] Rotary buffers */
    int64_t rope_rows;      /* >= row_len */
    float eps;              /* of the q / k norm; <= 0 -> FLT_EPSILON (F.rms_norm(eps=None) on fp32) */
    int32_t reserved0;      /* must be 0 */
    void *out;              /* [n_rows * row_len, dim] */
    void *saved;            /* 16-byte aligned; written by the forward, read by the backward */
    size_t saved_bytes;
    uint32_t *status;       /* optional, reserved: nothing in this call raises a status bit */
    void *workspace;        /* backward only, 16-byte aligned */
    size_t workspace_bytes;
} MotByteSelfAttnDesc;

/*
 * Backward: `fwd` as in the forward, with the `saved` buffer it filled.  Every non-null gradient is OVERWRITTEN.
 * dx, the gradient of the raw projections and d_lambda are written once per element / summed in a fixed order (the same bits on
 * every run); d_qkv_w and d_proj_w sum products over all byte positions with fp32 atomics.
 */
typedef struct MotByteSelfAttnGrads {
    uint32_t struct_size;  /* sizeof(MotByteSelfAttnGrads) */
    uint32_t reserved;
    const void *grad_out;  /* [n_rows * row_len, dim] */
    void *dx;              /* [n_rows * row_len, dim] */
    void *d_qkv_w;         /* [3, n_heads * 128, dim] */
    void *d_proj_w;        /* [dim, n_heads * 128] */
    float *d_lambda;       /* scalar */
} MotByteSelfAttnGrads;

size_t mot_byte_self_attn_desc_size(void);
size_t mot_byte_self_attn_saved_bytes(const MotByteSelfAttnDesc *desc /* host */);     /* 0 for a descriptor the call would refuse */
size_t mot_byte_self_attn_workspace_bytes(const MotByteSelfAttnDesc *desc /* host */); /* likewise */
int mot_byte_self_attn_fwd(const MotByteSelfAttnDesc *desc /* host */, mot_stream_t stream);
int mot_byte_self_attn_bwd(const MotByteSelfAttnDesc *fwd /* host */, const MotByteSelfAttnGrads *grads /* host */, mot_stream_t stream);

/*
 * Linear-on-bytes mixin, forward: replaces
 *   mixin_bytes(token_embs, byte_embs, byte_fc)         modded-nanogpt/runs/71051_mot-in_toks-valemb.py:225-229 (norm 130-131)
 *   on embed_tokens / embed_bytes at its call site      :312-314  (byte_fc: the parameter of :253, handed to Muon at :571)
 * Per token n of row-major (B, T), with K = bpt * byte_dim:
 *   u_n = cat_k byte_table[ids[n, k]]                   (the token's bpt byte rows side by side)
 *   x_n = rms_norm?(tok_table[tokens[n]] + byte_fc u_n)  byte_fc [model_dim, K], nn.Linear layout, no bias
 * tok_dim == model_dim; K need not equal model_dim.  No per-embedding norms, no learned scalars, one id tensor: the ids are
 * given (MOT_IDS_GIVEN, `ids`) or come from the token->byte table (MOT_IDS_FROM_TTB: tokens_to_bytes, then pull_dir), with the
 * int64 id outputs, counters and status word of MotEmbedMixDesc; out-of-range ids are clamped to row 0 and flagged.
 * MOT_F32: everything fp32, the product on the blocked fp32 MFMA summation of the other mixins.
 * MOT_BF16: tables, byte_fc, `out` and grad_out bf16, arithmetic fp32, rounded where the reference's bf16 run rounds:
 *   p = bf16(byte_fc u) (fp32 sums), s = bf16(tok + p), r = rsqrt(mean(s^2) + eps) in fp32, x = bf16(r s).
 * eps <= 0 means FLT_EPSILON for BOTH dtypes: F.rms_norm(eps=None) takes the epsilon of its fp32 opmath type on bf16 rows too (as
 * MotByteHeadDesc.eps); pass 2^-7 explicitly for torch.finfo(bfloat16).eps.
 * model_dim and K at most 2048; model_dim and byte_dim multiples of the 16-byte vector (4 fp32 / 8 bf16 elements).
 */
#define MOT_BYTE_FC_COMPOSED 1u /* MotByteFcMixDesc.flags, bf16 forward: the separate gather / product / row-pass kernels even where the one gather-GEMM qualifies */

typedef struct MotByteFcMixDesc {
    uint32_t struct_size;   /* sizeof(MotByteFcMixDesc), checked */
    int32_t dtype;          /* MotDType of tables / byte_fc / out */
    int64_t n_rows;         /* B */
    int64_t tokens_per_row; /* T */
    int32_t bpt;            /* byte slots per token */
    int32_t id_source;      /* MOT_IDS_FROM_TTB | MOT_IDS_GIVEN */
    const int32_t *tokens;  /* [B, T] */
    int32_t pull_dir;       /* MotPullDir           (FROM_TTB) */
    int32_t ttb_elem_bytes; /* 2 | 4                (FROM_TTB) */
    const void *ttb;        /* [ttb_rows, bpt]      (FROM_TTB) */
    int64_t ttb_rows;
    int32_t pad_byte, eot_byte;
    const int64_t *ids;     /* [B, T*bpt]           (GIVEN) */
    const void *tok_table;  /* [tok_rows, tok_dim] */
    int64_t tok_rows;
    int32_t tok_dim;        /* == model_dim */
    int32_t byte_dim;
    const void *byte_table; /* [byte_rows, byte_dim] */
    int64_t byte_rows;
    int32_t model_dim;
    int32_t norm_out;       /* 0: x = tok + byte_fc u */
    const void *byte_fc;    /* [model_dim, bpt*byte_dim] */
    float eps;              /* <= 0 -> FLT_EPSILON, both dtypes */
    uint32_t flags;         /* MOT_BYTE_FC_*; unknown bits are refused */
    void *out;              /* [B, T, model_dim] */
    float *out_row_rnorm;   /* optional [B, T] fp32: r of every row (1 without the norm); the fp32 backward needs it when norm_out */
    int64_t *out_ids_padded; /* optional [B, T*bpt] (FROM_TTB) */
    int64_t *out_ids_pulled; /* optional [B, T*bpt] (FROM_TTB) */
    int64_t *counters;      /* optional int64[4], as MotEmbedMixDesc.counters */
    uint32_t *status;       /* optional device word, see MOT_STATUS_* */
    void *workspace;        /* >= mot_byte_fc_mix_workspace_bytes (forward) / mot_byte_fc_mix_bwd_workspace_bytes (backward) */
    size_t workspace_bytes;
} MotByteFcMixDesc;

/*
 * Backward: `fwd` is the forward's descriptor with id_source == MOT_IDS_GIVEN (the ids the forward used); the id outputs and
 * counters are ignored.  With x = r s:
 *   ds = r (g - x (g.x) / model_dim)   (ds = g without the norm)
 *   d_tok[tokens[n]] += ds_n;   d_byte_fc += sum_n ds_n^T u_n;   du = ds byte_fc;   d_byte[ids[n,k]] += du_n[k*byte_dim ..]
 * u is gathered again.  MOT_F32 with norm_out reads the forward's x (`out`) and `out_row_rnorm`.  MOT_BF16 reads neither: a bf16 x
 * is three roundings away from the exact row, which would leave ds, and with it the token-table gradient, 2e-4 .. 8e-4 off; there
 * the product byte_fc u is formed again with its fp32 sums kept and s, r and x come from it in fp32 (one more product of the
 * forward's size; `out` and `out_row_rnorm` may be NULL).  Every gradient buffer is FP32 and ACCUMULATED into (+=), also with bf16
 * tables (there ds stays fp32 for the token table, and du and d_byte_fc run on the bf16 MFMA from bf16(ds) with fp32 sums).  Sums
 * use float atomics.
 */
typedef struct MotByteFcMixGrads {
    uint32_t struct_size;  /* sizeof(MotByteFcMixGrads) */
    uint32_t reserved;
    const void *grad_out;  /* [B, T, model_dim] in dtype */
    void *d_tok;           /* [tok_rows, model_dim]     fp32 */
    void *d_byte;          /* [byte_rows, byte_dim]     fp32 */
    void *d_byte_fc;       /* [model_dim, bpt*byte_dim] fp32 */
    const int32_t *token_order; /* optional: what mot_token_order wrote for fwd->tokens (same n_tokens, tok_rows) */
} MotByteFcMixGrads;

size_t mot_byte_fc_mix_desc_size(void);
size_t mot_byte_fc_mix_workspace_bytes(const MotByteFcMixDesc *desc /* host */);     /* 0 for a descriptor the call would refuse */
size_t mot_byte_fc_mix_bwd_workspace_bytes(const MotByteFcMixDesc *fwd /* host */);  /* likewise */
int mot_byte_fc_mix_fwd(const MotByteFcMixDesc *desc /* host */, mot_stream_t stream);
int mot_byte_fc_mix_bwd(const MotByteFcMixDesc *fwd /* host */, const MotByteFcMixGrads *grads /* host */, mot_stream_t stream);

/*
 * Bytes-only front-end and byte value embeddings, forward: replaces, in ONE launch for up to four tables indexed by one id stream,
 *   x = x0 = norm(reshape_bytes(embed_bytes(byte_inputs)))        modded-nanogpt/runs/5_bytes-in_bytes-valemb.py:225-232, 314 (runs 4, 6)
 *   ve = [reshape_bytes(value_embed(byte_inputs)) for value_embed in self.value_embeds_bytes]           :248, 305 (runs 2, 8)
 * There is no token row.  For every used slot j (n_out of them) and token n of row-major (B, T), with model_dim = bpt * byte_dim:
 *   out_j[n, k*byte_dim + c] = s_j[n] * table_j[ids[n, k], c],   s_j[n] = rsqrt(mean over the row of cat^2 + eps) if norm_j else 1
 * fp32 arithmetic, one rounding at the store for bf16; without a norm the row is a copy of the table rows, bit for bit.
 * The ids are given (MOT_IDS_GIVEN, `ids`; `tokens` may be NULL) or come from the token->byte table (MOT_IDS_FROM_TTB:
 * tokens_to_bytes, then pull_dir), with the int64 id outputs, counters and status word of MotEmbedMixDesc; an id outside a slot's
 * table reads that table's row 0 and raises MOT_STATUS_BYTE_OOR.
 * eps <= 0 means FLT_EPSILON for BOTH dtypes, as in MotByteFcMixDesc.
 * byte_dim a multiple of the 16-byte vector (4 fp32 / 8 bf16 elements), model_dim at most 2048, n_out in 1..4; every slot's dtype
 * equals the descriptor's.  The forward needs no workspace.
 */
#define MOT_BYTE_CAT_MAX_OUT 4

typedef struct MotByteCatSlot {
    const void *table; /* [rows, byte_dim] */
    int64_t rows;
    void *out;         /* [B, T, bpt*byte_dim]; ignored by the backward */
    int32_t norm;      /* 1: the row is rms-normalised over its model_dim columns */
    int32_t dtype;     /* MotDType of table and out: must equal MotByteCatDesc.dtype */
} MotByteCatSlot;

typedef struct MotByteCatDesc {
    uint32_t struct_size;   /* sizeof(MotByteCatDesc), checked */
    int32_t dtype;          /* MotDType of every table / out / grad_out */
    int64_t n_rows;         /* B */
    int64_t tokens_per_row; /* T */
    int32_t bpt;            /* byte slots per token */
    int32_t byte_dim;
    int32_t n_out;          /* used slots: 1 .. MOT_BYTE_CAT_MAX_OUT */
    int32_t id_source;      /* MOT_IDS_FROM_TTB | MOT_IDS_GIVEN */
    const int32_t *tokens;  /* [B, T]               (FROM_TTB) */
    const void *ttb;        /* [ttb_rows, bpt]      (FROM_TTB) */
    int64_t ttb_rows;
    int32_t ttb_elem_bytes; /* 2 | 4                (FROM_TTB) */
    int32_t pull_dir;       /* MotPullDir           (FROM_TTB) */
    int32_t pad_byte, eot_byte;
    const int64_t *ids;     /* [B, T*bpt]           (GIVEN) */
    float eps;              /* <= 0 -> FLT_EPSILON, both dtypes */
    uint32_t reserved0;     /* must be 0 */
    MotByteCatSlot slot[MOT_BYTE_CAT_MAX_OUT];
    int64_t *out_ids_padded; /* optional [B, T*bpt] (FROM_TTB) */
    int64_t *out_ids_pulled; /* optional [B, T*bpt] (FROM_TTB) */
    int64_t *counters;      /* optional int64[4], as MotEmbedMixDesc.counters */
    uint32_t *status;       /* optional device word, see MOT_STATUS_* */
    void *workspace;        /* backward only: >= mot_byte_cat_bwd_workspace_bytes */
    size_t workspace_bytes;
} MotByteCatDesc;

/*
 * Backward: `fwd` is the forward's descriptor with id_source == MOT_IDS_GIVEN (the ids the forward used or wrote); `out` and the id
 * outputs are ignored.  `counters`, when non-null, is a measurement aid here: int64[2], incremented by the number of non-zero
 * gradient terms added and by how many of them took the exact global path instead of the LDS sums.  Per used slot j whose grad_out is non-null (a null grad_out skips the slot):
 *   dcat = g                                  without the norm
 *   dcat = s (g - x (g.x) / model_dim)         with it, x = s cat gathered again and s recomputed
 *   d_table[ids[n, k], :] += dcat[n, k*byte_dim : (k+1)*byte_dim]
 * d_table is FP32 for both dtypes and ACCUMULATED into (+=).  Sums are privatised per workgroup in LDS as 64-bit fixed point and
 * flushed once per workgroup with float atomics: results depend on the order of those flushes in the last bits.
 */
typedef struct MotByteCatGradSlot {
    const void *grad_out; /* [B, T, bpt*byte_dim] in dtype, or NULL */
    void *d_table;        /* [rows, byte_dim] fp32 */
} MotByteCatGradSlot;

typedef struct MotByteCatGrads {
    uint32_t struct_size; /* sizeof(MotByteCatGrads) */
    uint32_t reserved;
    MotByteCatGradSlot slot[MOT_BYTE_CAT_MAX_OUT];
} MotByteCatGrads;

size_t mot_byte_cat_desc_size(void);
size_t mot_byte_cat_workspace_bytes(const MotByteCatDesc *desc /* host */);     /* 0: the forward needs none (and for a descriptor the call would refuse) */
size_t mot_byte_cat_bwd_workspace_bytes(const MotByteCatDesc *fwd /* host */);  /* 0 for a descriptor the call would refuse */
int mot_byte_cat_fwd(const MotByteCatDesc *desc /* host */, mot_stream_t stream);
int mot_byte_cat_bwd(const MotByteCatDesc *fwd /* host */, const MotByteCatGrads *grads /* host */, mot_stream_t stream);

/*
 * Token value embeddings: one to four tables of equal shape and dtype indexed by ONE token stream, which replaces
 *   self.value_embeds = nn.ModuleList([nn.Embedding(vocab_size, model_dim) for _ in range(3)])    scaled-pre-train/train_gpt.py:566
 *   ve = [value_embed(toks_in) for value_embed in self.value_embeds]                              scaled-pre-train/train_gpt.py:600
 * (modded-nanogpt/runs/71_*_toks-valemb.py:247 and :303, and every other *_toks-valemb.py run), forward and backward.
 * Forward, ONE launch for all tables: outs[j][n, :] = tables[j][tokens[n], :], a copy bit for bit; a position's id is read once;
 * no workspace.  An id outside [0, tok_rows) raises MOT_STATUS_TOKEN_OOR and reads row 0, as everywhere in the library.
 * dim a multiple of the 16-byte vector (4 fp32 / 8 bf16 elements) and at most 2048, tok_rows < 2^21 - 1 (the token order's limit),
 * n_tables in 1..MOT_VALUE_EMBEDS_MAX_TABLES: anything else is refused with MOT_EUNSUPPORTED before any launch.  Null pointers are
 * MOT_EINVAL; n_tokens == 0 is a no-op that returns MOT_OK.  Both calls are asynchronous on `stream` and never synchronise.
 */
#define MOT_VALUE_EMBEDS_MAX_TABLES 4

typedef struct MotValueEmbedsDesc {
    uint32_t struct_size;   /* sizeof(MotValueEmbedsDesc), checked */
    int32_t dtype;          /* MOT_F32 | MOT_BF16: every table, out, grad_out and d_table */
    int64_t n_tokens;       /* positions of the (flattened) token tensor, < 2^31 */
    const int32_t *tokens;  /* [n_tokens] */
    int64_t tok_rows;       /* rows of every table */
    int32_t dim;            /* columns of every table */
    int32_t n_tables;       /* 1 .. MOT_VALUE_EMBEDS_MAX_TABLES */
    const void *tables[MOT_VALUE_EMBEDS_MAX_TABLES]; /* [tok_rows, dim] each; the backward does not read them (may be NULL there) */
    void *outs[MOT_VALUE_EMBEDS_MAX_TABLES];         /* [n_tokens, dim] each; ignored by the backward */
    uint32_t *status;       /* optional device word, see MOT_STATUS_* */
    void *workspace;        /* backward only: >= mot_value_embeds_bwd_workspace_bytes, 16-byte aligned */
    size_t workspace_bytes;
} MotValueEmbedsDesc;

/*
 * Backward: the dense gradient of every table j whose grad_outs[j] is non-null (a null entry skips the table: its d_tables[j] is
 * not touched), in ONE call over one token order -- the caller's `token_order` (what mot_token_order wrote for the same tokens and
 * tok_rows) or one made inside the workspace:
 *   d_tables[j][r, :] = round_to_dtype(fp32 sum over the positions n with tokens[n] == r of grad_outs[j][n, :]),  +0 where r is absent.
 * Every element of every requested d_tables[j] is WRITTEN exactly once, in the tables' dtype, with plain stores: the caller zeroes
 * nothing (uninitialised memory is fine) and nothing is accumulated.  No atomic touches a gradient element.  The positions of an id
 * are summed in ascending position order, cut at fixed 64-position boundaries of the sorted stream; the pieces of a group that
 * crosses a boundary go to the workspace in fp32 and are added in ascending order by four waves, wave 0's share first.  The result
 * is the same bits on every run, with or without `token_order`.  All zeroing is done by kernels, so forward + backward capture
 * into a hipGraph.
 */
typedef struct MotValueEmbedsGrads {
    uint32_t struct_size; /* sizeof(MotValueEmbedsGrads) */
    uint32_t reserved;
    const void *grad_outs[MOT_VALUE_EMBEDS_MAX_TABLES]; /* [n_tokens, dim] in dtype, or NULL */
    void *d_tables[MOT_VALUE_EMBEDS_MAX_TABLES];        /* [tok_rows, dim] in dtype */
    const int32_t *token_order; /* optional, as MotEmbedMixGrads.token_order */
} MotValueEmbedsGrads;

size_t mot_value_embeds_desc_size(void);
size_t mot_value_embeds_bwd_workspace_bytes(const MotValueEmbedsDesc *fwd /* host */);   /* 0 for a descriptor the call would refuse */
int mot_value_embeds_fwd(const MotValueEmbedsDesc *desc /* host */, mot_stream_t stream);
int mot_value_embeds_bwd(const MotValueEmbedsDesc *fwd /* host */, const MotValueEmbedsGrads *grads /* host */, mot_stream_t stream);

/*
 * Mixture-of-tokenizers value embeddings: one to four slots, each a token value table, a byte value table and a mixin weight, over ONE
 * token stream and ONE byte-id stream, which replaces
 *   ve_tokens = [value_embed(token_inputs)[None] for value_embed in self.value_embeds_toks]
 *   ve_bytes = [value_embed(byte_inputs).squeeze()[None] for value_embed in self.value_embeds_bytes]
 *   ve = [mixin_bytes(vet, veb, vbmw) for vet, veb, vbmw in zip(ve_tokens, ve_bytes, self.value_byte_mixin_weights)]
 * of modded-nanogpt/runs/9_mot-in_mot-valemb.py:310-313 (mixin_bytes 225-235, parameters 252-254; runs 3 and 6 alike).
 * Per slot j and token n of row-major (B, T), with K = token_dim + bpt * byte_dim:
 *   u_j[n] = cat(tok_table_j[tokens[n]], byte_table_j[ids[n, 0]], ..., byte_table_j[ids[n, bpt-1]])
 *   y_j[n] = weight_j u_j[n]                       weight_j [out_dim, K], nn.Linear layout, no bias
 *   out_j[n] = rms_norm(y_j[n]) if norm_out else y_j[n]
 * The ids are in per-token byte order [B, T*bpt], given (MOT_IDS_GIVEN) or made ONCE for all slots from the token->byte table
 * (MOT_IDS_FROM_TTB: tokens_to_bytes, then pull_dir); an id outside a table reads row 0 and raises MOT_STATUS_TOKEN_OOR /
 * MOT_STATUS_BYTE_OOR.  All tables and weights share one dtype.  MOT_BF16: fp32 sums, rounded where the reference's bf16 run
 * rounds: y = bf16(W u), r = rsqrt(mean(y^2) + eps) in fp32, out = bf16(r y).  eps <= 0 means FLT_EPSILON for BOTH dtypes, as in
 * MotByteFcMixDesc.
 * Refused with MOT_EUNSUPPORTED before any launch: token_dim, byte_dim or out_dim not a multiple of the 16-byte vector (4 fp32 /
 * 8 bf16 elements), K or out_dim above 2048, n_slots outside 1..MOT_VALUE_MIX_MAX_SLOTS.  A wrong struct_size or a null slot
 * pointer is MOT_EINVAL.  An empty batch returns MOT_OK.  Every call is asynchronous on `stream`, allocates nothing and never
 * synchronises; all zeroing is done by kernels, so forward + backward capture into a hipGraph.
 */
#define MOT_VALUE_MIX_MAX_SLOTS 4

typedef struct MotValueMixSlot {
    const void *tok_table;  /* [tok_rows, token_dim] */
    const void *byte_table; /* [byte_rows, byte_dim] */
    const void *weight;     /* [out_dim, token_dim + bpt*byte_dim] */
    void *out;              /* [B, T, out_dim]; the backward reads it when norm_out */
    float *out_row_rnorm;   /* [B, T] fp32: r of every row.  Optional in the forward; the backward needs it when norm_out */
} MotValueMixSlot;

typedef struct MotValueMixDesc {
    uint32_t struct_size;   /* sizeof(MotValueMixDesc), checked */
    int32_t dtype;          /* MotDType of every table / weight / out / grad_out */
    int64_t n_rows;         /* B */
    int64_t tokens_per_row; /* T */
    int32_t bpt;            /* byte slots per token */
    int32_t id_source;      /* MOT_IDS_FROM_TTB | MOT_IDS_GIVEN */
    const int32_t *tokens;  /* [B, T] */
    int32_t pull_dir;       /* MotPullDir           (FROM_TTB) */
    int32_t ttb_elem_bytes; /* 2 | 4                (FROM_TTB) */
    const void *ttb;        /* [ttb_rows, bpt]      (FROM_TTB) */
    int64_t ttb_rows;
    int32_t pad_byte, eot_byte;
    const int64_t *ids;     /* [B, T*bpt]           (GIVEN) */
    int64_t tok_rows;       /* rows of every token value table */
    int64_t byte_rows;      /* rows of every byte value table */
    int32_t token_dim, byte_dim, out_dim;
    int32_t n_slots;        /* 1 .. MOT_VALUE_MIX_MAX_SLOTS */
    int32_t norm_out;       /* 0: out = y */
    float eps;              /* <= 0 -> FLT_EPSILON, both dtypes */
    MotValueMixSlot slot[MOT_VALUE_MIX_MAX_SLOTS];
    int64_t *out_ids;       /* optional [B, T*bpt] (FROM_TTB): the ids the tables were read with, what the backward wants as `ids` */
    uint32_t *status;       /* optional device word, see MOT_STATUS_* */
    void *workspace;        /* >= mot_value_mix_workspace_bytes(desc, backward), 16-byte aligned */
    size_t workspace_bytes;
} MotValueMixDesc;

/*
 * Backward: `fwd` is the forward's descriptor with id_source == MOT_IDS_GIVEN (the ids the forward used or wrote).  Per slot j
 * whose grad_out is non-null (a null grad_out skips the slot and touches none of its buffers), with x = out_j and r = out_row_rnorm_j:
 *   dy = r (g - x (g.x) / out_dim)        (dy = g without the norm)
 *   du = dy weight_j;   d_weight += dy^T u_j        u_j gathered again, slab by slab
 *   d_tok[r, :]  = round_to_dtype(fp32 sum of du[n, 0:token_dim] over the positions n with tokens[n] == r),  +0 where r is absent
 *   d_byte[ids[n, k], :] += du[n, token_dim + k*byte_dim : token_dim + (k+1)*byte_dim]
 * d_tok is WRITTEN exactly once, in the tables' dtype, with plain stores, under the contract of mot_value_embeds_bwd (the caller
 * zeroes nothing, the same bits on every run, with or without `token_order`); all slots share one token order -- the caller's or
 * one made in the workspace -- and one set of canonical positions.  d_byte and d_weight are FP32 for both dtypes and ACCUMULATED
 * into (+=) with float atomics (the byte tables through the LDS fixed-point sums of mot_byte_cat_bwd).  MOT_BF16: du and
 * d_weight run on the bf16 MFMA from bf16(dy) with fp32 sums; du stays fp32 on its way into the tables.  The workspace holds one
 * slot's rows plus the shared order, whatever n_slots is.
 */
typedef struct MotValueMixGradSlot {
    const void *grad_out; /* [B, T, out_dim] in dtype, or NULL */
    void *d_tok;          /* [tok_rows, token_dim]   in dtype, written once */
    void *d_byte;         /* [byte_rows, byte_dim]   fp32, += */
    void *d_weight;       /* [out_dim, K]            fp32, += */
} MotValueMixGradSlot;

typedef struct MotValueMixGrads {
    uint32_t struct_size; /* sizeof(MotValueMixGrads) */
    uint32_t reserved;
    MotValueMixGradSlot slot[MOT_VALUE_MIX_MAX_SLOTS];
    const int32_t *token_order; /* optional, as MotEmbedMixGrads.token_order */
} MotValueMixGrads;

size_t mot_value_mix_desc_size(void);
size_t mot_value_mix_workspace_bytes(const MotValueMixDesc *desc /* host */, int backward);   /* 0 for a descriptor the call would refuse */
int mot_value_mix_fwd(const MotValueMixDesc *desc /* host */, mot_stream_t stream);
int mot_value_mix_bwd(const MotValueMixDesc *fwd /* host */, const MotValueMixGrads *grads /* host */, mot_stream_t stream);

/*
 * The three input streams of modded-nanogpt/runs/71081_mot-in_toks-valemb.py:302-304, 315 in ONE call (every block of that run
 * reads x, x0t and x0b: :209-210, :319).  Per token n of row-major (B, T), with model_dim = bpt * byte_dim:
 *   x0t[n]                     = r_t tok_table[tokens[n]],         r_t = rsqrt(mean over model_dim of the row^2 + eps)
 *   x0b[n, k*byte_dim + c]     = r_k byte_table[ids[n, k], c],     r_k = rsqrt(mean over byte_dim of THAT byte row^2 + eps)
 *   x[n]                       = *scale_tok x0t[n] + *scale_byte x0b[n]                      (no outer norm)
 * Each of the three outputs may be NULL (not wanted); at least one is non-NULL.  The ids are in per-token byte order [B, T*bpt], given
 * (MOT_IDS_GIVEN) or made inside the kernel from the token->byte table (MOT_IDS_FROM_TTB: tokens_to_bytes, then pull_dir), with the
 * int64 id outputs, counters and status word of MotEmbedMixDesc; an id outside its table reads row 0 and raises MOT_STATUS_TOKEN_OOR /
 * MOT_STATUS_BYTE_OOR.  One dtype for tables, outputs and output gradients.  Arithmetic is fp32; MOT_BF16 is rounded where the
 * reference's eager bf16 run rounds: x0t = bf16(r_t a), x0b = bf16(r_k u), x = bf16(bf16(s_t x0t) + bf16(s_b x0b)) from the rounded
 * x0t and x0b.  scale_tok / scale_byte are DEVICE pointers to one fp32 each (the run's scalars[-1] / scalars[-2]) and are never read
 * on the host.  eps <= 0 means FLT_EPSILON for BOTH dtypes, as in MotByteFcMixDesc.
 * Refused with MOT_EUNSUPPORTED before any launch: model_dim != bpt * byte_dim, byte_dim not a multiple of the 16-byte vector (4 fp32
 * / 8 bf16 elements), model_dim above 2048, bpt outside 1..MOT_MAX_BPT, an unknown dtype, all three outputs NULL.  A wrong
 * struct_size or a null required pointer is MOT_EINVAL.  An empty batch returns MOT_OK.  Every call is asynchronous on `stream`,
 * allocates nothing, reads no environment variable and never synchronises; all zeroing is done by kernels, so forward + backward
 * capture into a hipGraph.  The forward's workspace holds the byte rows' rms factors (byte_rows fp32).
 */
typedef struct MotSplitX0Desc {
    uint32_t struct_size;   /* sizeof(MotSplitX0Desc), checked */
    int32_t dtype;          /* MOT_F32 | MOT_BF16: tables, outputs and output gradients */
    int64_t n_rows;         /* B */
    int64_t tokens_per_row; /* T */
    int32_t bpt;            /* byte slots per token */
    int32_t model_dim;      /* columns of tok_table and of every output: bpt * byte_dim */
    int32_t byte_dim;
    int32_t id_source;      /* MOT_IDS_FROM_TTB | MOT_IDS_GIVEN */
    const int32_t *tokens;  /* [B, T] */
    const void *ttb;        /* [ttb_rows, bpt]      (FROM_TTB) */
    int64_t ttb_rows;
    int32_t ttb_elem_bytes; /* 2 | 4                (FROM_TTB) */
    int32_t pull_dir;       /* MotPullDir           (FROM_TTB) */
    int32_t pad_byte, eot_byte;
    const int64_t *ids;     /* [B, T*bpt]           (GIVEN) */
    const void *tok_table;  /* [tok_rows, model_dim] */
    int64_t tok_rows;
    const void *byte_table; /* [byte_rows, byte_dim] */
    int64_t byte_rows;
    const float *scale_tok;  /* device, one fp32: scalars[-1] */
    const float *scale_byte; /* device, one fp32: scalars[-2] */
    float eps;              /* <= 0 -> FLT_EPSILON, both dtypes */
    uint32_t reserved0;     /* must be 0 */
    void *out_x0t;          /* [B, T, model_dim] or NULL; ignored by the backward, like the next two */
    void *out_x0b;
    void *out_x;
    int64_t *out_ids_padded; /* optional [B, T*bpt] (FROM_TTB) */
    int64_t *out_ids_pulled; /* optional [B, T*bpt] (FROM_TTB): with pull_dir the ids the byte table was read with, what the backward wants */
    int64_t *counters;      /* optional int64[4], as MotEmbedMixDesc.counters */
    uint32_t *status;       /* optional device word, see MOT_STATUS_* */
    void *workspace;        /* >= mot_splitx_workspace_bytes(desc, backward), 16-byte aligned */
    size_t workspace_bytes;
} MotSplitX0Desc;

/*
 * Backward: `fwd` is the forward's descriptor with id_source == MOT_IDS_GIVEN (the ids the forward used or wrote); the outputs are
 * not read, everything is computed again from the tables.  With h_t = grad_x0t + s_t grad_x and h_b = grad_x0b + s_b grad_x (a NULL
 * gradient is zero; at least one is non-NULL), y_k = r_k u_k:
 *   d a_n     = r_t (h_t - x0t (h_t . x0t) / model_dim)
 *   d u_{n,k} = r_k (h_b[k] - y_k (h_b[k] . y_k) / byte_dim)
 *   d_tok_table[r, :]  = round_to_dtype(fp32 sum of d a_n over the positions n with tokens[n] == r),  +0 where r is absent
 *   d_byte_table[ids[n, k], :] += d u_{n,k}
 *   *d_scale_tok = sum_n grad_x[n] . x0t[n],   *d_scale_byte = sum_n grad_x[n] . x0b[n]
 * Each of the four results may be NULL (not wanted).  d_tok_table is WRITTEN exactly once, in the tables' dtype, with plain stores,
 * under the contract of mot_value_embeds_bwd (the caller zeroes nothing, the same bits on every run, with or without
 * `token_order`); tok_rows >= 2^21 - 1 (the token order's limit) is refused with MOT_EUNSUPPORTED when it is asked for.  d_byte_table
 * is FP32 for both dtypes and ACCUMULATED into (+=) through the LDS fixed-point sums of mot_byte_cat_bwd.  The two scalars are
 * WRITTEN: per-workgroup partials over fixed ranges of 16 positions, added in order by one workgroup -- the same bits on every run.
 * The workspace holds d a of the whole batch (N x model_dim fp32), d u of one slab of 16 384 positions and the token order.
 */
typedef struct MotSplitX0Grads {
    uint32_t struct_size; /* sizeof(MotSplitX0Grads) */
    uint32_t reserved;
    const void *grad_x0t; /* [B, T, model_dim] in dtype, or NULL */
    const void *grad_x0b;
    const void *grad_x;
    void *d_tok_table;    /* [tok_rows, model_dim] in dtype, written once */
    void *d_byte_table;   /* [byte_rows, byte_dim] fp32, += */
    float *d_scale_tok;   /* one fp32, written */
    float *d_scale_byte;  /* one fp32, written */
    const int32_t *token_order; /* optional, as MotEmbedMixGrads.token_order */
} MotSplitX0Grads;

size_t mot_splitx_desc_size(void);
/* 0 for a descriptor the call would refuse on its shape, dtype or id source.  The query sees no pointers: a call whose three outputs
 * (or three gradients) are all NULL, or a backward that wants a token-table gradient at tok_rows >= 2^21 - 1, gets a size here and is
 * refused by the call itself. */
size_t mot_splitx_workspace_bytes(const MotSplitX0Desc *desc /* host */, int backward);
int mot_splitx_fwd(const MotSplitX0Desc *desc /* host */, mot_stream_t stream);
int mot_splitx_bwd(const MotSplitX0Desc *fwd /* host */, const MotSplitX0Grads *grads /* host */, mot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MOT_H_ */
