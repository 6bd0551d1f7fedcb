"""mixture-of-tokenizers_amd -- the mixture-of-tokenizers embedding front-end for MI355X (gfx950).

Hand-written HIP kernels behind a C ABI (include/mot.h, csrc/), called through ctypes.  The
Python layer mirrors the reference's interfaces for this path and nothing else:

  data_creation   make_embedding / tokens_to_bytes / pull_from_left / pull_from_right / create_batch
  functional      tensor-level wrappers (embed_mix = the fused gather + mix forward; byte_head_loss = the mixout byte head (one_call=True: split mode's step on one fused kernel); token_head_loss = the token-level head;
                  token_head_eval / byte_head_eval = the heads' evaluation form: per-row loss, top-1 prediction, target rank, counts;
                  plain_head_loss / plain_head_eval = the plain cross-entropy head (no softcap, ignore_index, mean over the kept targets)
                  of mathblations and inference, next_token = the generation step behind it (logits, top-k / top-p and the draw in one call), window_targets = its scored windows as ignored targets (max_kept / window_kept_bound: only the kept rows are scored);
                  byte_self_attn = the sliding-window byte self-attention layer of the concat mixin;
                  char_swa_step / char_swa_state = one decode step of the Llama character mixer with a device-side state,
                  char_ffn_step = the block's feed-forward on that step's rows;
                  byte_fc_mix = the linear-on-bytes mixin of run 71051; byte_cat = the bytes-only front-end and byte value embeddings
                  of runs 2, 4, 5, 6, 8; value_embeds = the token value embeddings of train_gpt.py:566/600 and the *_toks-valemb runs;
                  value_mix = the mixture-of-tokenizers value embeddings of runs 3, 6, 9;
                  split_x0 = run 71081's x0t, x0b and x in one call)
  modules         FlexibleEmbedding / ByteMixin* / CastedLinear (scaled-pre-train), DigitMixin* / GPTConfig / PlainLMHead
                  (mathblations), SumFrontEnd / ConcatFrontEnd / ByteFcFrontEnd / BytesFrontEnd / ValueEmbeds / MotValueEmbeds / SplitX0FrontEnd (modded-nanogpt), FusedFrontEnd (tokens -> x in one launch)
  loader          shard reader, rank slice, input/target shift (distributed_data_generator)
  grad_sync       GradBucket: one flat all-reduce for the front-end's gradients (train_gpt.py:1320-1321)

The directory name carries a hyphen; import it as ``mixture_of_tokenizers_amd`` (the loader
shim at the repo root maps that name onto this directory).
"""
from . import _capi
from . import data_creation, functional, grad_sync, loader, modules
from ._capi import build_info, check_status, set_debug_ids
from .modules import ByteFcFrontEnd, BytesFrontEnd, ConcatFrontEnd, MotValueEmbeds, PlainLMHead, SplitX0FrontEnd, ValueEmbeds
from .functional import CharSwaState, HeadEval, NextToken, byte_cat, byte_fc_mix, byte_head_eval, byte_head_loss, byte_self_attn, char_ffn_step, char_swa_state, char_swa_step, create_batch, embed_mix, embed_mix_plan, gather_rows, next_token, plain_head_eval, plain_head_loss, pull_bytes, split_x0, token_head_eval, token_head_loss, tokens_to_bytes, value_embeds, value_mix, window_kept_bound, window_targets

__all__ = [
    "build_info", "check_status", "set_debug_ids", "ByteFcFrontEnd", "BytesFrontEnd", "ConcatFrontEnd", "MotValueEmbeds", "PlainLMHead", "SplitX0FrontEnd", "ValueEmbeds", "data_creation", "functional", "grad_sync", "loader", "modules",
    "CharSwaState", "HeadEval", "NextToken", "byte_cat", "byte_fc_mix", "byte_head_eval", "byte_head_loss", "byte_self_attn", "char_ffn_step", "char_swa_state", "char_swa_step", "create_batch", "embed_mix", "embed_mix_plan", "gather_rows", "next_token", "plain_head_eval", "plain_head_loss", "pull_bytes", "split_x0", "token_head_eval", "token_head_loss", "tokens_to_bytes", "value_embeds", "value_mix", "window_kept_bound", "window_targets",
]
