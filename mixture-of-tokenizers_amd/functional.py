"""Tensor-level wrappers of the C ABI: shape/dtype/device checks, output allocation on the
caller's device and stream (torch caching allocator), then one call into libmot_hip.so.

Nothing here computes: every result comes from a HIP kernel.  Functions are wrapped in
``torch.compiler.disable`` so that a caller under ``torch.compile`` (train_gpt.py:1195) sees
them as opaque calls.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
import os
from dataclasses import dataclass
from typing import NamedTuple

import torch

from . import _capi as capi

# Kernel-selection switches, read ONCE at import (the C library itself reads no environment variable; the choice travels
# in MotEmbedMixDesc.flags).  Every call can override them with one_launch= / mean_generic= / du_fp32=.
_ENV_FLAGS = ((capi.FLAG_LINEAR_ONE_LAUNCH if os.environ.get("MOT_LIN_FUSED") else 0)
              | (capi.FLAG_MEAN_GENERIC if os.environ.get("MOT_NO_MEAN_LDS") else 0)
              | (capi.FLAG_BWD_DU_FP32 if os.environ.get("MOT_NO_DU16") else 0)
              | (capi.FLAG_LINEAR_COMPOSED if os.environ.get("MOT_LIN_COMPOSED") else 0))


def _flags(one_launch=None, mean_generic=None, du_fp32=None, composed=None) -> int:
    f = _ENV_FLAGS
    for bit, v in ((capi.FLAG_LINEAR_ONE_LAUNCH, one_launch), (capi.FLAG_MEAN_GENERIC, mean_generic), (capi.FLAG_BWD_DU_FP32, du_fp32),
                   (capi.FLAG_LINEAR_COMPOSED, composed)):
        if v is not None:
            f = (f | bit) if v else (f & ~bit)
    return f


_MODES = {"noop": capi.MIX_NOOP, "sum": capi.MIX_SUM, "mean": capi.MIX_MEAN, "concat_linear": capi.MIX_CONCAT_LINEAR,
          "concat": capi.MIX_CONCAT}
_PULLS = {None: capi.PULL_NONE, "none": capi.PULL_NONE, "left": capi.PULL_LEFT, "right": capi.PULL_RIGHT}


def _contig(t: torch.Tensor, dtype: torch.dtype, what: str) -> torch.Tensor:
    if t.dtype != dtype:
        raise TypeError(f"{what}: expected {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _table(t: torch.Tensor, what: str, like: torch.dtype | None = None) -> torch.Tensor:
    """fp32 (parity mode) or bf16 (what the training loop runs) table; all tables of a call agree."""
    capi.dtype_code(t.dtype)
    if like is not None and t.dtype != like:
        raise TypeError(f"{what}: {t.dtype} but the token table is {like}")
    return t if t.is_contiguous() else t.contiguous()


def _int_table(table: torch.Tensor, what: str) -> torch.Tensor:
    if table.dtype not in (torch.int16, torch.int32):
        raise TypeError(f"{what}: token->byte table must be int16 or int32, got {table.dtype}")
    if table.ndim != 2:
        raise ValueError(f"{what}: token->byte table must be (vocab, bytes_per_token)")
    return table if table.is_contiguous() else table.contiguous()


@torch.compiler.disable
def tokens_to_bytes(tokens: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """int64 byte ids of `tokens` (any shape) from an integer table (vocab, bpt) -> tokens.shape + (bpt,)."""
    table = _int_table(table, "tokens_to_bytes")
    dev = capi.require_device(tokens, table)
    tok = tokens.to(torch.int32) if tokens.dtype != torch.int32 else tokens
    tok = tok if tok.is_contiguous() else tok.contiguous()
    bpt = table.shape[1]
    out = torch.empty(tok.shape + (bpt,), dtype=torch.int64, device=dev)
    capi.check(capi.lib.mot_tokens_to_bytes(capi.ptr(tok), tok.numel(), capi.ptr(table), table.element_size(),
                                            table.shape[0], bpt, capi.ptr(out), capi.ptr(capi.status_word(dev)),
                                            capi.stream_of(dev)))
    capi.after_call(dev)
    return out


@torch.compiler.disable
def pull_bytes(byte_tensor: torch.Tensor, bytes_per_token: int, pad_byte: int, eot_byte: int, direction: str) -> torch.Tensor:
    """pull_from_left / pull_from_right on a (B, T) int64 tensor (data_creation.py:71-305)."""
    if byte_tensor.ndim != 2:
        raise ValueError("byte_tensor must be (B, T)")
    B, T = byte_tensor.shape
    if T == 0:
        return byte_tensor  # data_creation.py:82-83, 190
    dev = capi.require_device(byte_tensor)
    x = _contig(byte_tensor, torch.int64, "byte_tensor")
    out = torch.empty_like(x)
    capi.check(capi.lib.mot_pull_bytes(capi.ptr(x), capi.ptr(out), B, T, int(bytes_per_token), int(pad_byte),
                                       int(eot_byte), _PULLS[direction], capi.stream_of(dev)))
    return out


@torch.compiler.disable
def create_batch(tokens: torch.Tensor, table_left: torch.Tensor, table_right: torch.Tensor, pad_byte: int, eot_byte: int) -> torch.Tensor:
    """(B, T, 1+4*bpt) int64 packed batch (data_creation.py:308-330) in one launch."""
    tl, tr = _int_table(table_left, "create_batch"), _int_table(table_right, "create_batch")
    if tl.shape != tr.shape or tl.dtype != tr.dtype:
        raise ValueError("left/right tables must have the same shape and dtype")
    dev = capi.require_device(tokens, tl, tr)
    tok = _contig(tokens.to(torch.int32), torch.int32, "tokens")
    B, T = tok.shape
    bpt = tl.shape[1]
    out = torch.empty((B, T, 1 + 4 * bpt), dtype=torch.int64, device=dev)
    capi.check(capi.lib.mot_create_batch(capi.ptr(tok), B, T, capi.ptr(tl), capi.ptr(tr), tl.element_size(), tl.shape[0],
                                         bpt, int(pad_byte), int(eot_byte), capi.ptr(out),
                                         capi.ptr(capi.status_word(dev)), capi.stream_of(dev)))
    capi.after_call(dev)
    return out


@torch.compiler.disable
def char_matrix(codes: torch.Tensor, tok_offsets: torch.Tensor, seq_offsets: torch.Tensor, n_seqs: int, seq_len: int, max_char: int,
                leading_space: int, bos_token_id: int, eos_token_id: int) -> torch.Tensor:
    """(n_seqs, seq_len, max_char) int64 character ids (inference.py:56-67, 79-96); see mot_char_matrix in include/mot.h."""
    dev = capi.require_device(codes, tok_offsets, seq_offsets)
    c, to, so = _contig(codes, torch.int32, "codes"), _contig(tok_offsets, torch.int64, "tok_offsets"), _contig(seq_offsets, torch.int64, "seq_offsets")
    if so.numel() != n_seqs + 1:
        raise ValueError("seq_offsets must hold n_seqs + 1 entries")
    out = torch.empty((n_seqs, seq_len, max_char), dtype=torch.int64, device=dev)
    capi.check(capi.lib.mot_char_matrix(capi.ptr(c), capi.ptr(to), capi.ptr(so), int(n_seqs), int(seq_len), int(max_char), int(leading_space),
                                        int(bos_token_id), int(eos_token_id), capi.ptr(out), capi.stream_of(dev)))
    return out


@torch.compiler.disable
def gather_rows(table: torch.Tensor, ids: torch.Tensor, ids_b: torch.Tensor | None = None, *, rms_norm: bool = False,
                eps: float | None = None, scale: torch.Tensor | None = None) -> torch.Tensor:
    """scale * rms_norm?(table[ids] (+ table[ids_b])) -> ids.shape + (dim,)  (train_gpt.py:342-379)."""
    dev = capi.require_device(table, ids, ids_b, scale)
    tab = _table(table, "table")
    if ids.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"ids must be int32/int64, got {ids.dtype}")
    ia = ids if ids.is_contiguous() else ids.contiguous()
    ib = None
    if ids_b is not None:
        if ids_b.shape != ids.shape or ids_b.dtype != ids.dtype:
            raise ValueError("ids_b must match ids in shape and dtype")
        ib = ids_b if ids_b.is_contiguous() else ids_b.contiguous()
    out = torch.empty(ids.shape + (tab.shape[1],), dtype=tab.dtype, device=dev)
    capi.check(capi.lib.mot_gather_rows(capi.ptr(ia), capi.ptr(ib), ia.element_size(), ia.numel(), capi.ptr(tab),
                                        tab.shape[0], tab.shape[1], int(rms_norm), float(eps or 0.0), capi.ptr(scale),
                                        capi.ptr(out), capi.ptr(capi.status_word(dev)), capi.dtype_code(tab.dtype),
                                        capi.stream_of(dev)))
    capi.after_call(dev)
    return out


@dataclass
class MixResult:
    x: torch.Tensor
    ids_padded: torch.Tensor | None = None
    ids_pulled: torch.Tensor | None = None


_workspaces: dict[tuple[int, int], torch.Tensor] = {}
_retired: dict[tuple[int, int], list[torch.Tensor]] = {}


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor | None:
    """Per-(device, stream) scratch reused across calls (kernels on one stream are ordered).

    A captured hipGraph bakes the raw workspace pointer into its kernel nodes, so a buffer that a larger request
    replaces is NOT handed back to the allocator: it moves to a retired list and stays valid for whatever graph
    still points at it (workspaces only ever grow, geometrically, so the list holds a handful of buffers whose
    sizes sum to less than the live one).  `release_workspaces()` drops everything once no graph needs them."""
    if nbytes == 0:
        return None
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), capi.stream_of(dev))
    w = _workspaces.get(key)
    if w is None or w.numel() < nbytes:
        if w is not None:
            _retired.setdefault(key, []).append(w)
            nbytes = max(nbytes, 2 * w.numel())
        w = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
        _workspaces[key] = w
    return w


def release_workspaces() -> None:
    """Frees every library workspace (live and retired).  Call only when no captured graph that used them will be replayed."""
    _workspaces.clear()
    _retired.clear()


# ----------------------------------------------------------------------------------------------
# what the descriptor front-ends share: the token tensor, the byte-id source, the optional bindings, the call itself and the
# autograd nodes' common lines.  A new front-end is written on top of these ("Shared front-end pieces").
# ----------------------------------------------------------------------------------------------
def _int32(t: torch.Tensor) -> torch.Tensor:
    t = t.to(torch.int32) if t.dtype != torch.int32 else t
    return t if t.is_contiguous() else t.contiguous()


def _tokens_2d(tokens: torch.Tensor, what: str = "tokens must be (B, T) or (T,)") -> torch.Tensor:
    """tokens (B, T) or (T,) of any integer dtype -> the (B, T) int32 contiguous tensor the library reads; `what` is the refusal."""
    if tokens.ndim == 1:
        tokens = tokens[None]
    if tokens.ndim != 2:
        raise ValueError(what)
    tokens = tokens.to(torch.int32) if tokens.dtype != torch.int32 else tokens
    return tokens if tokens.is_contiguous() else tokens.contiguous()


def _bind_byte_ids(d, keep, *, B, T, bpt, ids, ttb, pull, what, ids_what="byte ids must hold bytes_per_token ids per token"):
    """The descriptor's byte-id source: the token->byte table `ttb` (+ `pull`) for the library to make the ids from, else the given
    int64 `ids`, which are returned (None with `ttb`: the caller allocates and binds whichever id outputs it wants back)."""
    if ttb is not None:
        tab = _int_table(ttb, what)
        if tab.shape[1] != bpt:
            raise ValueError(f"ttb has {tab.shape[1]} slots per token, bpt={bpt}")
        keep.append(tab)
        d.id_source, d.pull_dir = capi.IDS_FROM_TTB, _PULLS[pull]
        d.ttb, d.ttb_rows, d.ttb_elem_bytes = capi.ptr(tab), tab.shape[0], tab.element_size()
        return None
    if ids is None:
        raise ValueError("either ttb or ids must be given")
    ia = _contig(ids, torch.int64, "ids")
    if ia.numel() != B * T * bpt:
        raise ValueError(ids_what)
    keep.append(ia)
    d.id_source, d.ids = capi.IDS_GIVEN, capi.ptr(ia)
    return ia


def _new_ids(B, T, bpt, dev) -> torch.Tensor:
    return torch.empty((B, T * bpt), dtype=torch.int64, device=dev)


def _bind_counters(d, counters, dev) -> None:
    if counters is not None:
        if counters.dtype != torch.int64 or counters.numel() < 4 or counters.device != dev:
            raise ValueError("counters must be an int64[4] tensor on the inputs' device")
        d.counters = capi.ptr(counters)


def _bind_token_order(gr, keep, token_order, n_tokens, tok_rows, dev, contiguous="contiguous ") -> None:
    if token_order is not None:
        need = capi.lib.mot_token_order_ints(n_tokens, int(tok_rows))
        if token_order.dtype != torch.int32 or token_order.numel() != need or token_order.device != dev or not token_order.is_contiguous():
            raise ValueError(f"token_order must be the {contiguous}int32[{need}] tensor token_order(tokens, {tok_rows}) returned")
        gr.token_order = capi.ptr(token_order)
        keep.append(token_order)


def _launch(dev, d, fn, *extra, ws_bytes=None):
    """The tail of every descriptor call: the device's status word, the workspace (`ws_bytes`: the library's size query, called with
    the descriptor), `fn(desc, *extra, stream)` on the current stream, its return code and the deferred status check.  `fn` None
    binds only (embed_mix_plan launches later).  Returns the workspace."""
    d.status = capi.ptr(capi.status_word(dev))
    ws = None if ws_bytes is None else _workspace(dev, ws_bytes(C.byref(d)))
    if ws is not None:
        d.workspace, d.workspace_bytes = capi.ptr(ws), ws.numel()
    if fn is not None:
        capi.check(fn(C.byref(d), *extra, capi.stream_of(dev)))
        capi.after_call(dev)
    return ws


def _ready_order(ctx_order, device):
    """The token order an autograd node asked for beside its forward, made ready for the backward on `device`'s current stream
    (None: the backward groups the positions itself)."""
    if ctx_order is None:
        return None
    order, ev = ctx_order
    cur = torch.cuda.current_stream(device)
    if ev is not None:
        cur.wait_event(ev)
    order.record_stream(cur)
    return order


def _grad_like(g, p):
    """The fp32 gradient sums rounded once to the parameter's dtype, in its shape."""
    return None if g is None else g.to(p.dtype).reshape(p.shape)


@torch.compiler.disable
def _embed_mix_fwd(tokens: torch.Tensor, tok_table: torch.Tensor, byte_table: torch.Tensor | None = None, *,
              mode: str, bpt: int = 0,
              ttb: torch.Tensor | None = None, pull: str | None = None, add_padded: bool = False,
              pad_byte: int = 456, eot_byte: int = 457,
              ids_a: torch.Tensor | None = None, ids_b: torch.Tensor | None = None,
              weight: torch.Tensor | None = None, bias: torch.Tensor | None = None, bytes_first: bool = False,
              norm_tok: bool = False, norm_byte: bool = False, norm_out: bool = False, eps: float | None = None,
              scale_tok: torch.Tensor | None = None, scale_byte: torch.Tensor | None = None,
              out: torch.Tensor | None = None, return_ids: bool = False,
              counters: torch.Tensor | None = None, row_rnorm: torch.Tensor | None = None,
              one_launch: bool | None = None, mean_generic: bool | None = None, composed: bool | None = None,
              _plan: bool = False) -> torch.Tensor | MixResult:
    """One fused launch of mot_embed_mix_fwd; see include/mot.h for the per-token formula.

    tokens (B, T) integer.  Byte ids either come from `ttb` (+ `pull` = "left" | "right" | None,
    + `add_padded`) inside the kernel, or are given as `ids_a` / `ids_b` (B, T*bpt) int64.
    `scale_*` are 0-dim/1-element DEVICE tensors (learned scalars are read on the device).
    mode "concat" (x = cat(token row, byte rows), runs/711_*.py:224-232) takes no `weight`; its output has
    tok_dim + bpt * byte_dim columns.
    `composed` (bf16 concat_linear: the separate gather / GEMM / norm kernels instead of the one gather-GEMM),
    `one_launch` (concat_linear: the one-launch tile kernel instead of the composed kernels) and `mean_generic` (mean: the
    whole-row kernel instead of the LDS column-slice kernel) override the import-time defaults (MotEmbedMixDesc.flags).
    """
    m = _MODES[mode]
    tok = _tokens_2d(tokens)
    dev = capi.require_device(tokens, tok_table, byte_table, ttb, ids_a, ids_b, weight, bias, scale_tok, scale_byte)
    for what, sc in (("scale_tok", scale_tok), ("scale_byte", scale_byte)):
        if sc is not None and (sc.dtype != torch.float32 or sc.numel() != 1):
            raise TypeError(f"{what}: expected a 1-element float32 device tensor, got {sc.dtype} x {sc.numel()}")
    B, T = tok.shape
    tt = _table(tok_table, "tok_table")
    fdt = tt.dtype
    d = capi.MotEmbedMixDesc()
    d.struct_size = C.sizeof(capi.MotEmbedMixDesc)
    d.dtype = capi.dtype_code(fdt)
    d.flags = _flags(one_launch, mean_generic, composed=composed)
    d.n_rows, d.tokens_per_row, d.bpt, d.mode = B, T, int(bpt), m
    d.tokens = capi.ptr(tok)
    d.tok_table, d.tok_rows, d.tok_dim = capi.ptr(tt), tt.shape[0], tt.shape[1]
    keep = [tok, tt]
    ids_padded = ids_pulled = None
    if m != capi.MIX_NOOP:
        if byte_table is None:
            raise ValueError("byte_table is required unless mode == 'noop'")
        bt = _table(byte_table, "byte_table", fdt)
        keep.append(bt)
        d.byte_table, d.byte_rows, d.byte_dim = capi.ptr(bt), bt.shape[0], bt.shape[1]
        if ttb is not None:
            tab = _int_table(ttb, "embed_mix")
            if tab.shape[1] != bpt:
                raise ValueError(f"ttb has {tab.shape[1]} slots per token, bpt={bpt}")
            keep.append(tab)
            d.id_source, d.pull_dir = capi.IDS_FROM_TTB, _PULLS[pull]
            d.ttb, d.ttb_rows, d.ttb_elem_bytes = capi.ptr(tab), tab.shape[0], tab.element_size()
            d.add_padded = int(add_padded)
            if return_ids:
                ids_padded, ids_pulled = _new_ids(B, T, bpt, dev), _new_ids(B, T, bpt, dev)
                d.out_ids_padded, d.out_ids_pulled = capi.ptr(ids_padded), capi.ptr(ids_pulled)
        else:
            if ids_a is None:
                raise ValueError("either ttb or ids_a must be given")
            ia = _contig(ids_a, torch.int64, "ids_a")
            assert ia.numel() == B * T * bpt, "byte ids must hold bytes_per_token ids per token"
            keep.append(ia)
            d.id_source, d.ids_a = capi.IDS_GIVEN, capi.ptr(ia)
            if ids_b is not None:
                ib = _contig(ids_b, torch.int64, "ids_b")
                assert ib.numel() == ia.numel()
                keep.append(ib)
                d.ids_b = capi.ptr(ib)
    d.pad_byte, d.eot_byte = int(pad_byte), int(eot_byte)
    if m == capi.MIX_CONCAT_LINEAR:
        if weight is None:
            raise ValueError("weight is required for mode == 'concat_linear'")
        w = _table(weight, "weight", fdt)
        keep.append(w)
        d.weight, d.model_dim = capi.ptr(w), w.shape[0]
        if w.shape[1] != tt.shape[1] + bpt * d.byte_dim:
            raise ValueError(f"weight has {w.shape[1]} input features, expected {tt.shape[1]} + {bpt}*{d.byte_dim}")
        if bias is not None:
            bs = _table(bias, "bias", fdt)
            keep.append(bs)
            d.bias = capi.ptr(bs)
        d.bytes_first = int(bytes_first)
    else:
        if m == capi.MIX_CONCAT and (weight is not None or bias is not None):
            raise ValueError("mode == 'concat' is the pure concatenation: it takes no weight / bias (see 'concat_linear')")
        # "concat": x = cat(token row, byte rows), runs/711_*.py:224-232
        d.model_dim = tt.shape[1] + int(bpt) * d.byte_dim if m == capi.MIX_CONCAT else tt.shape[1]
    d.norm_tok, d.norm_byte, d.norm_out = int(norm_tok), int(norm_byte), int(norm_out)
    d.eps = float(eps or 0.0)
    d.scale_tok, d.scale_byte = capi.ptr(scale_tok), capi.ptr(scale_byte)
    if out is None:
        out = torch.empty((B, T, d.model_dim), dtype=fdt, device=dev)
    else:
        if out.shape != (B, T, d.model_dim) or out.dtype != fdt or not out.is_contiguous() or out.device != dev:
            raise ValueError("out must be a contiguous (B, T, model_dim) tensor of the tables' dtype on their device")
    d.out = capi.ptr(out)
    _bind_counters(d, counters, dev)
    if row_rnorm is not None:   # (B, T) fp32, written by the concat_linear kernel when norm_out (saved for the backward)
        assert row_rnorm.dtype == torch.float32 and row_rnorm.numel() == B * T and row_rnorm.is_contiguous()
        d.out_row_rnorm = capi.ptr(row_rnorm)
    result = MixResult(out, ids_padded, ids_pulled) if return_ids else out
    if _plan:
        ws = _launch(dev, d, None, ws_bytes=capi.lib.mot_embed_mix_workspace_bytes)
        return EmbedMixPlan(d, keep + [ws, out, ids_padded, ids_pulled, counters, row_rnorm, scale_tok, scale_byte], dev, result)
    _launch(dev, d, capi.lib.mot_embed_mix_fwd, ws_bytes=capi.lib.mot_embed_mix_workspace_bytes)
    return result


class EmbedMixPlan:
    """A validated, fully bound descriptor of one fused-forward call: ``plan()`` is a single C call on the
    current stream (a few microseconds of host time instead of the ~50 us the checked wrapper spends),
    reading the CURRENT contents of the bound tensors (update tokens / tables in place between calls).
    Build with :func:`embed_mix_plan`; forward only (no autograd)."""

    def __init__(self, desc, keepalive, device, result):
        self._d, self._keep, self._dev, self.result = desc, keepalive, device, result
        self._ref = C.byref(desc)

    def __call__(self):
        rc = capi.lib.mot_embed_mix_fwd(self._ref, torch.cuda.current_stream(self._dev).cuda_stream)
        if rc:
            capi.check(rc)
        return self.result


def embed_mix_plan(tokens, tok_table, byte_table=None, **kw) -> EmbedMixPlan:
    """Same arguments as :func:`embed_mix`; returns an :class:`EmbedMixPlan` instead of launching."""
    return _embed_mix_fwd(tokens, tok_table, byte_table, _plan=True, **kw)


@torch.compiler.disable
def token_order(tokens: torch.Tensor, tok_rows: int) -> torch.Tensor:
    """One call of mot_token_order: the batch's positions grouped by token id (opaque int32 buffer), which the table-gradient
    scatter of every backward over these tokens walks.  Depends on `tokens` only; runs on the current stream."""
    dev = capi.require_device(tokens)
    tok = _int32(tokens)
    order = torch.empty(capi.lib.mot_token_order_ints(tok.numel(), int(tok_rows)), dtype=torch.int32, device=dev)
    capi.check(capi.lib.mot_token_order(capi.ptr(tok), tok.numel(), int(tok_rows), capi.ptr(order), capi.ptr(capi.status_word(dev)),
                                        capi.stream_of(dev)))
    capi.after_call(dev)
    return order


class _TokenOrderCache:
    """The token order of the last few token tensors seen by the autograd node, produced BESIDE the forward: on a side stream that
    waits for the tokens and runs while the forward kernel streams (the sort is three small latency-bound kernels, the forward is
    HBM-bound), so the backward finds it ready instead of spending 0.08 ms of a 0.55 ms call on it.  One order serves every
    backward over the same tokens: several embedding tables indexed by one token tensor (modded-nanogpt/runs/71_*.py value
    embeddings), gradient accumulation, the two front-ends of a mixin/mixout pair.  An entry is valid for the SAME tensor object
    at the SAME version with the same table height; entries keep their token tensor alive (a few MB), so an address cannot be
    reused under a stale entry."""

    def __init__(self, keep: int = 4):
        self.keep, self.entries, self.side = keep, [], {}

    def get(self, tokens: torch.Tensor, tok_rows: int):
        # Inside a graph capture the cache is neither read nor written: the sort is captured in line on the capturing stream.  An
        # entry made eagerly would be replayed as it is after tokens.copy_(new batch) (the graph does not re-sort) and carries an
        # event recorded outside the capture; an entry made here would hand later eager calls a buffer that only replays refresh.
        if torch.cuda.is_current_stream_capturing():
            return token_order(tokens, tok_rows), None
        for e in self.entries:
            if e[0] is tokens and e[1] == tokens._version and e[2] == tok_rows:
                return e[3], e[4]
        dev = tokens.device
        cur = torch.cuda.current_stream(dev)
        side = self.side.get(dev.index)
        if side is None:
            side = self.side[dev.index] = torch.cuda.Stream(device=dev)
        side.wait_stream(cur)                              # the tokens are ready when the current stream gets here
        with torch.cuda.stream(side):
            order = token_order(tokens, tok_rows)
            ev = torch.cuda.Event()
            ev.record(side)
        self.entries.insert(0, (tokens, tokens._version, tok_rows, order, ev))
        del self.entries[self.keep:]
        return order, ev

    def clear(self):
        self.entries.clear()


_token_orders = _TokenOrderCache()
_HOIST_SORT = not os.environ.get("MOT_NO_ORDER_HOIST")            # dev switch: let every backward group the positions itself


_BWD_MODES = ("sum", "noop", "concat_linear", "mean", "concat")


class _EmbedMixFn(torch.autograd.Function):
    """Autograd node of the fused front-end: forward = one mot_embed_mix_fwd launch, backward = one
    mot_embed_mix_bwd launch (dense gradients, like nn.Embedding(sparse=False) in the reference)."""

    @staticmethod
    def forward(ctx, tok_table, byte_table, scale_tok, scale_byte, weight, bias, tokens, kw):
        kw = dict(kw)
        mode = kw["mode"]
        want_ids = kw.get("ttb") is not None and mode != "noop"
        user_return_ids = kw.pop("return_ids", False)
        kw.pop("weight", None); kw.pop("bias", None)
        rn = None
        if mode == "concat_linear" and kw.get("norm_out"):
            t2 = tokens if tokens.ndim == 2 else tokens[None]
            rn = torch.empty(t2.shape, dtype=torch.float32, device=tok_table.device)
        r = _embed_mix_fwd(tokens, tok_table.detach(), None if byte_table is None else byte_table.detach(),
                           scale_tok=None if scale_tok is None else scale_tok.detach(),
                           scale_byte=None if scale_byte is None else scale_byte.detach(),
                           weight=None if weight is None else weight.detach(), bias=None if bias is None else bias.detach(),
                           return_ids=want_ids or user_return_ids, row_rnorm=rn, **kw)
        x = r.x if isinstance(r, MixResult) else r
        ids_a, ids_b = kw.get("ids_a"), kw.get("ids_b")
        if want_ids:   # the byte ids the kernel produced in LDS, written out once for the backward
            ids_a = r.ids_pulled if kw.get("pull") not in (None, "none") else r.ids_padded
            ids_b = r.ids_padded if kw.get("add_padded") else None
        # the positions grouped by token id, for the backward: requested here so that it runs beside the forward launch above
        ctx.order = _token_orders.get(tokens, tok_table.shape[0]) if _HOIST_SORT else None
        ctx.save_for_backward(tok_table, byte_table, scale_tok, scale_byte, tokens, ids_a, ids_b, weight, bias,
                              x if mode == "concat_linear" else None, rn)
        ctx.kw = {k: kw[k] for k in ("mode", "bpt", "norm_tok", "norm_byte", "norm_out", "eps", "bytes_first") if k in kw}
        if user_return_ids:
            ctx.mark_non_differentiable(r.ids_padded, r.ids_pulled)
            return x, r.ids_padded, r.ids_pulled
        return x

    @staticmethod
    def backward(ctx, gx, *_):
        tok_table, byte_table, scale_tok, scale_byte, tokens, ids_a, ids_b, weight, bias, x, rn = ctx.saved_tensors
        # Parameters whose .grad is managed by grad_sync.GradBucket (an explicit opt-in: GradBucket(..., in_place=True) marks them)
        # take the kernel's += directly (mot_embed_mix_bwd only ever adds into its outputs): no temporary table-sized gradient,
        # no zero fill, no AccumulateGrad pass over it.  The price, documented on GradBucket: for those parameters autograd sees
        # no gradient -- tensor hooks and post-accumulate-grad hooks do not fire, and torch.autograd.grad(...) would find .grad
        # changed -- so the direct path is refused under torch.autograd.grad (ctx.needs_input_grad is all there is to go by: it is
        # taken only when backward() was asked to accumulate into leaves).  Everything else gets a fresh fp32 gradient handed to
        # autograd as usual.
        direct = {k: p.grad for k, p in (("tok_table", tok_table), ("byte_table", byte_table), ("weight", weight), ("bias", bias))
                  if _accumulates_in_place(p)}
        g = embed_mix_backward(gx, tokens, tok_table.detach(), None if byte_table is None else byte_table.detach(),
                               ids_a=ids_a, ids_b=ids_b, token_order=_ready_order(ctx.order, gx.device),
                               scale_tok=None if scale_tok is None else scale_tok.detach(),
                               scale_byte=None if scale_byte is None else scale_byte.detach(),
                               weight=None if weight is None else weight.detach(), bias=None if bias is None else bias.detach(),
                               out=None if x is None else x.detach(), row_rnorm=rn, into=direct, **ctx.kw)
        def like(k, p):  # bf16 parameters get their gradient rounded once, from the fp32 sums
            return None if p is None or k in direct else _grad_like(g.get(k), p)
        return (like("tok_table", tok_table), like("byte_table", byte_table), like("scale_tok", scale_tok),
                like("scale_byte", scale_byte), like("weight", weight), like("bias", bias), None, None)


def _accumulates_in_place(p) -> bool:
    """True for a leaf parameter that grad_sync.GradBucket has bound to its flat buffer: fp32, contiguous .grad present."""
    if p is None or not getattr(p, "_mot_grad_in_place", False) or not p.requires_grad or not p.is_leaf:
        return False
    gr = p.grad
    return gr is not None and gr.dtype == torch.float32 and gr.is_contiguous() and gr.shape == p.shape and gr.device == p.device


@torch.compiler.disable
def embed_mix_backward(grad_out: torch.Tensor, tokens: torch.Tensor, tok_table: torch.Tensor, byte_table: torch.Tensor | None = None, *,
                       mode: str, bpt: int = 0, ids_a: torch.Tensor | None = None, ids_b: torch.Tensor | None = None,
                       norm_tok: bool = False, norm_byte: bool = False, norm_out: bool = False, eps: float | None = None,
                       scale_tok: torch.Tensor | None = None, scale_byte: torch.Tensor | None = None,
                       weight: torch.Tensor | None = None, bias: torch.Tensor | None = None, bytes_first: bool = False,
                       out: torch.Tensor | None = None, row_rnorm: torch.Tensor | None = None,
                       into: dict | None = None, du_fp32: bool | None = None, one_launch: bool | None = None,
                       token_order: torch.Tensor | None = None) -> dict:
    """One launch of mot_embed_mix_bwd.  Returns dense fp32 gradients {tok_table, byte_table, scale_tok,
    scale_byte, weight, bias} -- fp32 also when the tables are bfloat16 (accumulated in fp32; the autograd
    node rounds once to the parameter dtype); pass `into` (same keys, fp32) to accumulate into existing
    buffers such as ``param.grad``.  `token_order`: what :func:`token_order` returned for these tokens and this table height (the
    caller orders streams); without it the call groups the positions itself."""
    m = _MODES[mode]
    if tokens.ndim == 1:
        tokens = tokens[None]
    dev = capi.require_device(grad_out, tokens, tok_table, byte_table, ids_a, ids_b, scale_tok, scale_byte)
    tok = _int32(tokens)
    B, T = tok.shape
    dt = tok_table.dtype
    code = capi.dtype_code(dt)
    tt = _contig(tok_table, dt, "tok_table")
    g = _contig(grad_out, dt, "grad_out")
    d = capi.MotEmbedMixDesc()
    d.struct_size = C.sizeof(capi.MotEmbedMixDesc)
    d.dtype = code
    d.flags = _flags(one_launch=one_launch, du_fp32=du_fp32)
    d.n_rows, d.tokens_per_row, d.bpt, d.mode = B, T, int(bpt), m
    d.tokens = capi.ptr(tok)
    d.tok_table, d.tok_rows, d.tok_dim, d.model_dim = capi.ptr(tt), tt.shape[0], tt.shape[1], tt.shape[1]
    into = into or {}
    fwd_out = out
    out = {"tok_table": into.get("tok_table", None), "byte_table": into.get("byte_table", None),
           "scale_tok": into.get("scale_tok", None), "scale_byte": into.get("scale_byte", None)}
    if out["tok_table"] is None:
        out["tok_table"] = torch.zeros_like(tt, dtype=torch.float32)
    keep = [tok, tt, g]
    gr = capi.MotEmbedMixGrads()
    gr.struct_size = C.sizeof(capi.MotEmbedMixGrads)
    gr.grad_out = capi.ptr(g)
    gr.d_tok_table = capi.ptr(out["tok_table"])
    if m != capi.MIX_NOOP:
        bt = _contig(byte_table, dt, "byte_table")
        ia = _contig(ids_a, torch.int64, "ids_a")
        keep += [bt, ia]
        d.byte_table, d.byte_rows, d.byte_dim = capi.ptr(bt), bt.shape[0], bt.shape[1]
        d.id_source, d.ids_a = capi.IDS_GIVEN, capi.ptr(ia)
        if ids_b is not None:
            ib = _contig(ids_b, torch.int64, "ids_b")
            keep.append(ib)
            d.ids_b = capi.ptr(ib)
        if out["byte_table"] is None:
            out["byte_table"] = torch.zeros_like(bt, dtype=torch.float32)
        gr.d_byte_table = capi.ptr(out["byte_table"])
    if m == capi.MIX_CONCAT:
        d.model_dim = tt.shape[1] + int(bpt) * bt.shape[1]
    if m == capi.MIX_CONCAT_LINEAR:
        w = _contig(weight, dt, "weight")
        keep.append(w)
        d.weight, d.model_dim, d.bytes_first = capi.ptr(w), w.shape[0], int(bytes_first)
        out["weight"] = into.get("weight") if into.get("weight") is not None else torch.zeros_like(w, dtype=torch.float32)
        gr.d_weight = capi.ptr(out["weight"])
        if bias is not None:
            bs = _contig(bias, dt, "bias")
            keep.append(bs)
            d.bias = capi.ptr(bs)
            out["bias"] = into.get("bias") if into.get("bias") is not None else torch.zeros_like(bs, dtype=torch.float32)
            gr.d_bias = capi.ptr(out["bias"])
        if norm_out:
            if fwd_out is None or row_rnorm is None:
                raise ValueError("concat_linear backward with norm_out needs the forward's output and row_rnorm")
            xo = _contig(fwd_out, dt, "out")
            keep.append(xo)
            d.out, d.out_row_rnorm = capi.ptr(xo), capi.ptr(row_rnorm)
    d.norm_tok, d.norm_byte, d.norm_out = int(norm_tok), int(norm_byte), int(norm_out)
    d.eps = float(eps or 0.0)
    d.scale_tok, d.scale_byte = capi.ptr(scale_tok), capi.ptr(scale_byte)
    for k, sc in (("scale_tok", scale_tok), ("scale_byte", scale_byte)):
        if sc is not None and out[k] is None:
            out[k] = torch.zeros(1, dtype=torch.float32, device=dev)
    gr.d_scale_tok, gr.d_scale_byte = capi.ptr(out["scale_tok"]), capi.ptr(out["scale_byte"])
    _bind_token_order(gr, keep, token_order, B * T, tt.shape[0], dev)
    _launch(dev, d, capi.lib.mot_embed_mix_bwd, C.byref(gr), ws_bytes=capi.lib.mot_embed_mix_bwd_workspace_bytes)
    return out


_ONCE_MODES = ("sum", "noop", "concat")


def _write_once_refusal(kw) -> str | None:
    """Why mot_embed_mix_bwd_once would refuse these forward arguments (None: it takes them)."""
    pre = "mixture-of-tokenizers_amd: embed_mix(write_once=True): "
    mode = kw.get("mode")
    if mode not in _ONCE_MODES:
        return pre + f"mode '{mode}' is not built (embed_mix_bwd_once covers 'sum', 'noop' and 'concat'); use write_once=False"
    if mode != "noop" and (kw.get("ids_b") is not None or kw.get("add_padded")):
        return pre + "a second id tensor (ids_b / add_padded) is not built (embed_mix_bwd_once takes one id tensor); use write_once=False"
    return None


@torch.compiler.disable
def embed_mix_backward_once(grad_out: torch.Tensor, tokens: torch.Tensor, tok_table: torch.Tensor, byte_table: torch.Tensor | None = None, *,
                            mode: str, bpt: int = 0, ids_a: torch.Tensor | None = None,
                            norm_tok: bool = False, norm_byte: bool = False, norm_out: bool = False, eps: float | None = None,
                            scale_tok: torch.Tensor | None = None, scale_byte: torch.Tensor | None = None,
                            token_order: torch.Tensor | None = None, out: dict | None = None, want_grads=None) -> dict:
    """One call of mot_embed_mix_bwd_once.  Returns {tok_table (the table's dtype), byte_table (fp32), scale_tok, scale_byte (fp32)}:
    every element written by the call (the byte table is cleared by a kernel first), so `out=` may name `torch.empty` buffers of those
    dtypes and shapes.  The token-table gradient is the fp32 sum in ascending position order, rounded once, +0 where an id does not
    occur: the same bits on every run.  `want_grads`: the keys to compute (default: all that apply); `token_order` as in
    :func:`embed_mix_backward`."""
    refusal = _write_once_refusal({"mode": mode})
    if refusal:
        raise NotImplementedError(refusal)
    m = _MODES[mode]
    if tokens.ndim == 1:
        tokens = tokens[None]
    dev = capi.require_device(grad_out, tokens, tok_table, byte_table, ids_a, scale_tok, scale_byte)
    tok = _int32(tokens)
    B, T = tok.shape
    dt = tok_table.dtype
    tt = _contig(tok_table, dt, "tok_table")
    g = _contig(grad_out, dt, "grad_out")
    d = capi.MotEmbedMixDesc()
    d.struct_size = C.sizeof(capi.MotEmbedMixDesc)
    d.dtype = capi.dtype_code(dt)
    d.n_rows, d.tokens_per_row, d.bpt, d.mode = B, T, int(bpt), m
    d.tokens = capi.ptr(tok)
    d.tok_table, d.tok_rows, d.tok_dim, d.model_dim = capi.ptr(tt), tt.shape[0], tt.shape[1], tt.shape[1]
    keep = [tok, tt, g]
    shapes = {"tok_table": (tt.shape, dt)}
    if m != capi.MIX_NOOP:
        if byte_table is None or ids_a is None:
            raise ValueError("byte_table and ids_a are required unless mode == 'noop'")
        bt = _contig(byte_table, dt, "byte_table")
        ia = _contig(ids_a, torch.int64, "ids_a")
        if ia.numel() != B * T * int(bpt):
            raise ValueError("byte ids must hold bytes_per_token ids per token")
        keep += [bt, ia]
        d.byte_table, d.byte_rows, d.byte_dim = capi.ptr(bt), bt.shape[0], bt.shape[1]
        d.id_source, d.ids_a = capi.IDS_GIVEN, capi.ptr(ia)
        shapes["byte_table"] = (bt.shape, torch.float32)
        if m == capi.MIX_CONCAT:
            d.model_dim = tt.shape[1] + int(bpt) * bt.shape[1]
    if g.numel() != B * T * d.model_dim:
        raise ValueError(f"grad_out must hold (B, T, {d.model_dim}) elements")
    d.norm_tok, d.norm_byte, d.norm_out = int(norm_tok), int(norm_byte), int(norm_out)
    d.eps = float(eps or 0.0)
    d.scale_tok, d.scale_byte = capi.ptr(scale_tok), capi.ptr(scale_byte)
    for k, sc in (("scale_tok", scale_tok), ("scale_byte", scale_byte)):
        if sc is not None:
            if sc.dtype != torch.float32 or sc.numel() != 1:
                raise TypeError(f"{k}: expected a 1-element float32 device tensor, got {sc.dtype} x {sc.numel()}")
            shapes[k] = ((1,), torch.float32)
    want = set(shapes) if want_grads is None else set(want_grads)
    if not want <= set(shapes):
        raise ValueError(f"want_grads {sorted(want - set(shapes))} do not apply to this call (it has {sorted(shapes)})")
    out = dict(out or {})
    res = {}
    for k in ("tok_table", "byte_table", "scale_tok", "scale_byte"):
        if k not in want:
            continue
        shape, kdt = shapes[k]
        buf = out.get(k)
        if buf is None:
            buf = torch.empty(shape, dtype=kdt, device=dev)
        elif buf.dtype != kdt or buf.numel() != math.prod(shape) or not buf.is_contiguous() or buf.device != dev:
            raise ValueError(f"out['{k}'] must be a contiguous {kdt} tensor of {tuple(shape)} on the inputs' device")
        res[k] = buf
    gr = capi.MotEmbedMixGradsOnce()
    gr.struct_size = C.sizeof(capi.MotEmbedMixGradsOnce)
    gr.grad_out = capi.ptr(g)
    gr.d_tok_table, gr.d_byte_table = capi.ptr(res.get("tok_table")), capi.ptr(res.get("byte_table"))
    gr.d_scale_tok, gr.d_scale_byte = capi.ptr(res.get("scale_tok")), capi.ptr(res.get("scale_byte"))
    _bind_token_order(gr, keep, token_order, B * T, tt.shape[0], dev)
    _launch(dev, d, capi.lib.mot_embed_mix_bwd_once, C.byref(gr), ws_bytes=capi.lib.mot_embed_mix_bwd_once_workspace_bytes)
    return res


class _EmbedMixOnceFn(torch.autograd.Function):
    """Autograd node of the fused front-end with the write-once backward: forward = the launch of _EmbedMixFn, backward = one
    mot_embed_mix_bwd_once call, whose token-table gradient is handed to autograd in the parameter's dtype as it stands."""

    @staticmethod
    def forward(ctx, tok_table, byte_table, scale_tok, scale_byte, tokens, kw):
        return _EmbedMixFn.forward(ctx, tok_table, byte_table, scale_tok, scale_byte, None, None, tokens, kw)

    @staticmethod
    def backward(ctx, gx, *_):
        tok_table, byte_table, scale_tok, scale_byte, tokens, ids_a = ctx.saved_tensors[:6]
        params = {"tok_table": tok_table, "byte_table": byte_table, "scale_tok": scale_tok, "scale_byte": scale_byte}
        want = [k for i, k in enumerate(params) if params[k] is not None and ctx.needs_input_grad[i]]
        kw = {k: v for k, v in ctx.kw.items() if k != "bytes_first"}
        g = embed_mix_backward_once(gx, tokens, tok_table.detach(), None if byte_table is None else byte_table.detach(),
                                    ids_a=ids_a, token_order=_ready_order(ctx.order, gx.device),
                                    scale_tok=None if scale_tok is None else scale_tok.detach(),
                                    scale_byte=None if scale_byte is None else scale_byte.detach(), want_grads=want, **kw)
        return tuple(_grad_like(g.get(k), p) if p is not None else None for k, p in params.items()) + (None, None)


def embed_mix(tokens: torch.Tensor, tok_table: torch.Tensor, byte_table: torch.Tensor | None = None, *,
              scale_tok: torch.Tensor | None = None, scale_byte: torch.Tensor | None = None, write_once: bool = False, **kw):
    """The fused front-end (see `_embed_mix_fwd` for the arguments).  With autograd enabled and
    differentiable parameters it records one backward node: modes "sum", "noop", "concat", "concat_linear" with
    float32 or bfloat16 tables; "mean" without an output norm.  Anything else raises here,
    at forward time, rather than in backward().

    `write_once=True` (modes "sum", "noop", "concat", one id tensor) gives the node the write-once backward
    (:func:`embed_mix_backward_once`): the token-table gradient arrives in the parameter's dtype, written once from fp32 sums in
    ascending position order -- no zeroed fp32 buffer, no atomics on it, no rounding pass, the same bits on every run -- and the
    GradBucket in-place `+=` path is never taken.  What that call does not build raises NotImplementedError here."""
    if write_once:
        refusal = _write_once_refusal(kw)
        if refusal:
            raise NotImplementedError(refusal)
    params = (tok_table, byte_table, scale_tok, scale_byte, kw.get("weight"), kw.get("bias"))
    if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in params):
        if kw["mode"] not in _BWD_MODES:
            raise RuntimeError(
                f"mixture-of-tokenizers_amd: backward of mode '{kw['mode']}' is not built yet (forward only); "
                "call it under torch.no_grad() or with frozen parameters")
        if kw["mode"] == "mean" and kw.get("norm_out"):
            raise RuntimeError(
                "mixture-of-tokenizers_amd: the backward of the MEAN mix is built without an output norm (the reference's residual, "
                "inference.py:267, has none; mot_embed_mix_bwd, include/mot.h); call it under torch.no_grad() or with frozen parameters")
        if kw.get("out") is not None or kw.get("counters") is not None:
            raise ValueError("out= / counters= cannot be combined with autograd")
        if write_once:
            r = _EmbedMixOnceFn.apply(tok_table, byte_table, scale_tok, scale_byte, tokens, kw)
        else:
            r = _EmbedMixFn.apply(tok_table, byte_table, scale_tok, scale_byte, kw.get("weight"), kw.get("bias"), tokens, kw)
        if kw.get("return_ids"):
            return MixResult(*r)
        return r
    return _embed_mix_fwd(tokens, tok_table, byte_table, scale_tok=scale_tok, scale_byte=scale_byte, **kw)


def _cross_attn_desc(tokens, ids_a, ids_b, tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, cos_q, sin_q, cos_k, sin_k,
                     bpt, n_heads, norm_tok, norm_byte, head_layout, eps, matmul=None, widened=None, wide_cache=None):
    """Validated MotCrossAttnDesc for both directions; returns (desc, keepalive list, device, T, D).  `widened`: the fp32 copies
    (tables, weights, lambda) an earlier call of the same autograd node made of the same bf16 operands -- keep[1:7] -- reused
    instead of made again."""
    dev = capi.require_device(tokens, ids_a, ids_b, tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, cos_q, sin_q, cos_k, sin_k)
    T = tokens.shape[1]
    tok = _int32(tokens)
    f32 = torch.float32
    # bf16 tables (the production cast, train_gpt.py:1124-1126): the attention kernels of this mixin are fp32, so the operands are
    # widened once per call -- the tables as they are (bf16 values), the fp32 master weights rounded to bf16 first, as
    # `self.q_w.type_as(x)` does (lines 277-278, 185-186) -- and the result is rounded once to bf16 by the caller.  The products
    # over the tokens (q, c_proj and their four backward products) then run on the bf16 MFMA (`matmul_dtype`, include/mot.h):
    # their row operands are bf16 tensors in the reference too.  `matmul="fp32"` keeps them on the fp32 MFMA.
    bf = tok_table.dtype == torch.bfloat16
    if matmul not in (None, "fp32", "bf16"):
        raise ValueError(f"cross_attn: matmul must be None, 'fp32' or 'bf16' (got {matmul!r})")
    mm_bf16 = (bf and tok_table.shape[1] % 8 == 0) if matmul is None else matmul == "bf16"
    if byte_table.dtype != tok_table.dtype:
        raise TypeError(f"cross_attn: byte table is {byte_table.dtype} but the token table is {tok_table.dtype}")
    wide = (lambda t: t.detach().float()) if bf else (lambda t: t.detach())
    as_used = (lambda w: w.detach().to(torch.bfloat16).float()) if bf else (lambda w: w.detach())
    if bf and wide_cache is not None:   # no-grad calls with a caller-kept cache: the fp32 copies live beside the K / V tables
        def _kept(fn):
            def get(t):
                key = (t.data_ptr(), t._version, tuple(t.shape), str(t.dtype))
                hit = wide_cache.get(id(t))
                if hit is None or hit[0] != key:
                    hit = wide_cache[id(t)] = (key, fn(t), t)
                return hit[1]
            return get
        wide, as_used = _kept(wide), _kept(as_used)
    if widened is not None:   # (the backward of a bf16 step: the forward's copies; autograd has checked that the originals are unchanged)
        wide = as_used = None
        tt, bt = widened[0], widened[1]
    else:
        tt, bt = _contig(wide(tok_table), f32, "tok_table"), _contig(wide(byte_table), f32, "byte_table")
    D = tt.shape[1]
    if bt.shape[1] != D:
        raise AssertionError("cross_attn: byte_dim == token_dim == model_dim (train_gpt.py:449)")
    HD = n_heads * 128
    if widened is not None:
        qw, kvw, pw = widened[2], widened[3], widened[4]
    else:
        qw, kvw, pw = _contig(as_used(q_w), f32, "q_w"), _contig(as_used(kv_w), f32, "kv_w"), _contig(as_used(proj_w), f32, "proj_w")
    if qw.shape != (HD, D) or kvw.shape != (2, HD, D) or pw.shape != (D, HD):
        raise AssertionError(f"cross_attn: weights {tuple(qw.shape)}, {tuple(kvw.shape)}, {tuple(pw.shape)} do not fit heads={n_heads}, dim={D}")
    lam = widened[5] if widened is not None else _contig(as_used(lambda_factor).reshape(1), f32, "lambda_factor")
    ia = _contig(ids_a.reshape(-1), torch.int64, "ids_a")
    ib = None if ids_b is None else _contig(ids_b.reshape(-1), torch.int64, "ids_b")
    if ia.numel() != T * bpt or (ib is not None and ib.numel() != T * bpt):
        raise AssertionError(f"cross_attn: byte ids must hold T*bpt = {T * bpt} entries")
    rot = [_contig(t, f32, "rotary buffer") for t in (cos_q, sin_q, cos_k, sin_k)]
    if any(r.ndim != 2 or r.shape[1] != 64 for r in rot):
        raise AssertionError("cross_attn: rotary buffers must be (len, 64)")
    d = capi.MotCrossAttnDesc()
    d.struct_size = C.sizeof(capi.MotCrossAttnDesc)
    d.dtype, d.n_tokens, d.bpt, d.n_heads, d.dim = capi.F32, T, int(bpt), int(n_heads), D
    d.matmul_dtype = capi.BF16 if mm_bf16 else capi.F32
    d.io_dtype = capi.BF16 if (bf and mm_bf16) else capi.F32   # bf16 tables: the result and its gradient cross the boundary in bf16
    tt16 = None
    if bf and mm_bf16:   # the bf16 table itself: the normalised token rows are then gathered in bf16 directly
        tt16 = _contig(tok_table.detach(), torch.bfloat16, "tok_table")
        d.tok_table_bf16 = capi.ptr(tt16)
    d.head_layout = {"as_viewed": capi.HEADS_AS_VIEWED, "per_token": capi.HEADS_PER_TOKEN}[head_layout]
    d.tokens, d.ids_a, d.ids_b = capi.ptr(tok), capi.ptr(ia), capi.ptr(ib)
    d.tok_table, d.tok_rows, d.byte_table, d.byte_rows = capi.ptr(tt), tt.shape[0], capi.ptr(bt), bt.shape[0]
    d.norm_tok, d.norm_byte = int(norm_tok), int(norm_byte)
    d.q_w, d.kv_w, d.proj_w, d.lambda_factor = capi.ptr(qw), capi.ptr(kvw), capi.ptr(pw), capi.ptr(lam)
    d.cos_q, d.sin_q, d.cos_k, d.sin_k = (capi.ptr(r) for r in rot)
    d.rot_q_len, d.rot_k_len = rot[0].shape[0], rot[2].shape[0]
    # norm() is F.rms_norm(x, eps=None): eps = finfo(x.dtype).eps, and with bf16 tables every tensor it is applied to here (the
    # embeddings, q, k) is bf16 in the reference -- 2^-7, not the float32 epsilon of the widened copies (train_gpt.py:172-173)
    d.eps = float(eps or (2.0 ** -7 if bf else 0.0))
    return d, [tok, tt, bt, qw, kvw, pw, lam, ia, ib] + rot + [tt16], dev, T, D


class _CrossAttnFn(torch.autograd.Function):
    """One autograd node for the cross-attention mixin: forward = mot_cross_attn_fwd, backward = mot_cross_attn_bwd
    (everything is recomputed from the inputs; dense fp32 gradients for the two tables, q_w, kv_w, c_proj and lambda)."""

    @staticmethod
    def forward(ctx, tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, tokens, ids_a, ids_b, rot, kw):
        # the projected queries and the attention output are kept for the backward (2 x T x hdim floats)
        saved = torch.empty(2 * tokens.shape[-1] * kw["n_heads"] * 128, dtype=torch.float32, device=tok_table.device)
        ctx.save_for_backward(tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, tokens, ids_a, saved, *rot)
        ctx.ids_b = ids_b          # (an integer tensor or None: nothing autograd tracks)
        ctx.kw = kw
        # bf16 tables: the fp32 copies of the operands this call makes serve the backward too (six conversions less per step)
        ctx.widened = [] if tok_table.dtype == torch.bfloat16 else None
        x = _cross_attn_fwd(tokens, ids_a, ids_b, tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, *rot, saved_qy=saved, _keep_widened=ctx.widened, **kw)
        return x.to(tok_table.dtype)

    @staticmethod
    def backward(ctx, gx):
        tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, tokens, ids_a, saved, cq, sq, ck, sk = ctx.saved_tensors
        g = cross_attn_backward(gx, tokens, ids_a, tok_table, byte_table, q_w=q_w, kv_w=kv_w, proj_w=proj_w, lambda_factor=lambda_factor,
                                cos_q=cq, sin_q=sq, cos_k=ck, sin_k=sk, saved_qy=saved, ids_b=ctx.ids_b, widened=ctx.widened or None, **ctx.kw)
        # fp32 sums; the tables' gradients are rounded once to the tables' dtype (bf16 in production), the weights stay fp32 masters
        return (g["tok_table"].to(tok_table.dtype), g["byte_table"].to(byte_table.dtype), g["q_w"], g["kv_w"], g["proj_w"],
                g["lambda_factor"].reshape(lambda_factor.shape).to(lambda_factor.dtype), None, None, None, None, None)


@torch.compiler.disable
def cross_attn_backward(grad_out, tokens, ids_a, tok_table, byte_table, *, q_w, kv_w, proj_w, lambda_factor, cos_q, sin_q, cos_k, sin_k,
                        bpt, n_heads, norm_tok=True, norm_byte=True, head_layout="as_viewed", eps=None, saved_qy=None, ids_b=None,
                        matmul=None, widened=None) -> dict:
    """One call of mot_cross_attn_bwd: dense fp32 gradients {tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor}.
    `saved_qy`: the buffer the forward filled (projected queries + attention output); without it they are recomputed.
    `ids_b`: the second id tensor of the add_padded_and_pulled embedding (train_gpt.py:364-372)."""
    if tokens.ndim == 1:
        tokens = tokens[None]
    d, keep, dev, T, D = _cross_attn_desc(tokens, ids_a, ids_b, tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, cos_q, sin_q, cos_k, sin_k,
                                          bpt, n_heads, norm_tok, norm_byte, head_layout, eps, matmul, widened)
    io = torch.bfloat16 if d.io_dtype == capi.BF16 else torch.float32
    g = _contig(grad_out.reshape(T, D).to(io), io, "grad_out")
    out = {"tok_table": torch.zeros_like(keep[1]), "byte_table": torch.zeros_like(keep[2]), "q_w": torch.zeros_like(keep[3]),
           "kv_w": torch.zeros_like(keep[4]), "proj_w": torch.zeros_like(keep[5]), "lambda_factor": torch.zeros(1, dtype=torch.float32, device=dev)}
    gr = capi.MotCrossAttnGrads()
    gr.struct_size = C.sizeof(capi.MotCrossAttnGrads)
    gr.grad_out = capi.ptr(g)
    gr.d_tok_table, gr.d_byte_table = capi.ptr(out["tok_table"]), capi.ptr(out["byte_table"])
    gr.d_q_w, gr.d_kv_w, gr.d_proj_w, gr.d_lambda = capi.ptr(out["q_w"]), capi.ptr(out["kv_w"]), capi.ptr(out["proj_w"]), capi.ptr(out["lambda_factor"])
    if saved_qy is not None:
        d.saved_qy = capi.ptr(_contig(saved_qy, torch.float32, "saved_qy"))
    _launch(dev, d, capi.lib.mot_cross_attn_bwd, C.byref(gr), ws_bytes=capi.lib.mot_cross_attn_bwd_workspace_bytes)
    return out


def _cross_attn_fwd(tokens, ids_a, ids_b, tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, cos_q, sin_q, cos_k, sin_k, *,
                    bpt, n_heads, norm_tok=True, norm_byte=True, head_layout="as_viewed", eps=None, kv_cache=None, saved_qy=None, matmul=None,
                    _keep_widened=None):
    d, keep, dev, T, D = _cross_attn_desc(tokens, ids_a, ids_b, tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, cos_q, sin_q, cos_k, sin_k,
                                          bpt, n_heads, norm_tok, norm_byte, head_layout, eps, matmul,
                                          wide_cache=None if kv_cache is None else kv_cache.setdefault("widened", {}))
    if _keep_widened is not None:
        _keep_widened.extend(keep[1:7])   # tt, bt, qw, kvw, pw, lam
    out = torch.empty((1, T, D), dtype=torch.bfloat16 if d.io_dtype == capi.BF16 else torch.float32, device=dev)
    d.out = capi.ptr(out)
    if saved_qy is not None:
        d.saved_qy = capi.ptr(saved_qy)
    if kv_cache is not None and ids_b is None:
        # the per-byte-row key / value tables depend on (byte_table, kv_w, lambda_factor) only: kept across calls while those are unchanged
        key = tuple((t.data_ptr(), t._version) for t in (byte_table, kv_w, lambda_factor)) + (bool(norm_byte), float(eps or 0.0), str(dev))
        n = 2 * keep[2].shape[0] * n_heads * 128
        if kv_cache.get("buf") is None or kv_cache["buf"].numel() != n or kv_cache["buf"].device != dev:
            kv_cache["buf"], kv_cache["key"] = torch.empty(n, dtype=torch.float32, device=dev), None
        d.kv_tables, d.kv_tables_ready = capi.ptr(kv_cache["buf"]), int(kv_cache.get("key") == key)
        kv_cache["key"] = key
    _launch(dev, d, capi.lib.mot_cross_attn_fwd, ws_bytes=capi.lib.mot_cross_attn_workspace_bytes)
    return out


@torch.compiler.disable
def cross_attn(tokens: torch.Tensor, ids_a: torch.Tensor, tok_table: torch.Tensor, byte_table: torch.Tensor, *,
               q_w: torch.Tensor, kv_w: torch.Tensor, proj_w: torch.Tensor, lambda_factor: torch.Tensor,
               cos_q: torch.Tensor, sin_q: torch.Tensor, cos_k: torch.Tensor, sin_k: torch.Tensor,
               bpt: int, n_heads: int, ids_b: torch.Tensor | None = None, norm_tok: bool = True, norm_byte: bool = True,
               head_layout: str = "as_viewed", eps: float | None = None, kv_cache: dict | None = None,
               matmul: str | None = None) -> torch.Tensor:
    """The cross-attention byte mixin on top of the two embedding gathers (train_gpt.py:342-379, 446-464, 271-300):
    tokens (1, T) -> (1, T, dim).  The reference asserts batch 1 (line 275).  fp32.  With autograd enabled and
    differentiable parameters it records one backward node (either embedding: one id tensor, or norm(emb(padded) + emb(pulled))).
    head_layout "as_viewed" reproduces the reference's reshape of k and v (lines 283-284); "per_token" is the
    rearrange its comment names.  bfloat16 tables are accepted (operands widened once per call, bf16 result and table gradients):
    the attention itself stays fp32, the products over the tokens -- q, c_proj and their backward products -- then run on the
    bf16 MFMA with fp32 accumulation, their row operands rounded to bf16 where the reference's are bf16 tensors
    (`matmul="fp32"` keeps them on the fp32 MFMA; `matmul="bf16"` asks for the bf16 MFMA with fp32 tables too)."""
    if tokens.ndim == 1:
        tokens = tokens[None]
    assert tokens.shape[0] == 1, "Must use batch size = 1 for FlexAttention"      # train_gpt.py:275
    kw = dict(bpt=bpt, n_heads=n_heads, norm_tok=norm_tok, norm_byte=norm_byte, head_layout=head_layout, eps=eps, matmul=matmul)
    params = (tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _CrossAttnFn.apply(tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, tokens, ids_a, ids_b, (cos_q, sin_q, cos_k, sin_k), kw)
    # `kv_cache` (a dict the caller keeps, e.g. on the module): inference calls reuse the per-byte-row K/V tables while the
    # byte table, kv_w and lambda_factor are unchanged (tensor versions are checked)
    return _cross_attn_fwd(tokens, ids_a, ids_b, tok_table, byte_table, q_w, kv_w, proj_w, lambda_factor, cos_q, sin_q, cos_k, sin_k,
                           kv_cache=kv_cache, **kw).to(tok_table.dtype)


_SWA_VERSIONS = {"no_residual": capi.SWA_NO_RESIDUAL, "one_residual": capi.SWA_ONE_RESIDUAL, "two_residual": capi.SWA_TWO_RESIDUAL}


@torch.compiler.disable
def char_swa(tokens: torch.Tensor, char_ids: torch.Tensor, tok_table: torch.Tensor, char_table: torch.Tensor, *,
             attn_norm_w: torch.Tensor, char_norm_w: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, wo: torch.Tensor,
             n_heads: int, head_dim: int, window: int = 8, norm_eps: float = 1e-5, version: str = "two_residual",
             lambda_tok: torch.Tensor | None = None, lambda_char: torch.Tensor | None = None, matmul: str | None = None,
             kv_cache: dict | None = None) -> torch.Tensor:
    """The Llama character mixer up to the feed-forward (inference.py:146-224 + 260-267 on the gathers of 323-327):
    tokens (B, T) int, char_ids (B, T, c_v) int64 -> h (B, T, dim) fp32.  bf16 tables: bf16 result; operands widened once, the
    attention in fp32, the two products over the tokens (wq, wo) on the bf16 MFMA with their row operands rounded to bf16
    (`matmul="fp32"` keeps them on the fp32 MFMA, `matmul="bf16"` asks for the bf16 MFMA with fp32 tables).  Forward only (the
    file is the reference's inference path); see mot_char_swa_fwd in include/mot.h.  `kv_cache` (a dict the caller keeps, e.g. on
    the module): the per-character key / value tables are reused across calls while char_table, char_norm_w, wk and wv are unchanged
    (storage and version are checked)."""
    if matmul not in (None, "fp32", "bf16"):
        raise ValueError(f"char_swa: matmul must be None, 'fp32' or 'bf16' (got {matmul!r})")
    if tokens.ndim == 1:
        tokens, char_ids = tokens[None], char_ids[None]
    if char_ids.ndim != 3 or char_ids.shape[:2] != tokens.shape:
        raise ValueError(f"char_ids must be (B, T, c_v) matching tokens {tuple(tokens.shape)}, got {tuple(char_ids.shape)}")
    kv_key = tuple((t.data_ptr(), t._version) for t in (char_table, char_norm_w, wk, wv)) + (float(norm_eps), str(char_table.dtype))
    params = (tok_table, char_table, attn_norm_w, char_norm_w, wq, wk, wv, wo, lambda_tok, lambda_char)
    if torch.is_grad_enabled() and any(p is not None and p.requires_grad for p in params):
        raise RuntimeError("mixture-of-tokenizers_amd: the character mixer (inference/inference.py) is built forward-only; call it under "
                           "torch.no_grad() or with frozen parameters")
    dev = capi.require_device(tokens, char_ids, *params)
    f32 = torch.float32
    tok = _contig(tokens.to(torch.int32), torch.int32, "tokens")
    cid = _contig(char_ids, torch.int64, "char_ids")
    B, T = tok.shape
    # bfloat16 tables / weights (round 3; the reference script itself runs in the default float32): every operand is widened once
    # per call -- the values a bf16 model holds -- the arithmetic is the fp32 kernels', and the result is rounded once to bf16
    bf = tok_table.dtype == torch.bfloat16
    if bf:
        if char_table.dtype != torch.bfloat16:
            raise TypeError(f"char_swa: char_table is {char_table.dtype} but the token table is bfloat16")
        # (with `kv_cache` the widened copies are kept beside the tables while the originals are unchanged: the file is an inference
        #  path, and the Llama token table alone is 0.5 GB to read and 1 GB to write per call otherwise)
        wide_cache = None if kv_cache is None else kv_cache.setdefault("widened", {})

        def widen(t):
            if t is None:
                return None
            if wide_cache is None:
                return t.detach().to(torch.bfloat16).float()
            key = (t.data_ptr(), t._version, tuple(t.shape), str(t.dtype))
            hit = wide_cache.get(id(t))
            if hit is None or hit[0] != key:
                hit = wide_cache[id(t)] = (key, t.detach().to(torch.bfloat16).float(), t)   # (t itself: the id stays its own)
            return hit[1]
        tok_table, char_table, attn_norm_w, char_norm_w, wq, wk, wv, wo, lambda_tok, lambda_char = (
            widen(t) for t in (tok_table, char_table, attn_norm_w, char_norm_w, wq, wk, wv, wo, lambda_tok, lambda_char))
    tt, ct = _contig(tok_table.detach(), f32, "tok_table"), _contig(char_table.detach(), f32, "char_table")
    D, hdim = tt.shape[1], n_heads * head_dim
    if ct.shape[1] != D:
        raise ValueError("char_table and tok_table must have the same number of columns (hidden_size)")
    ws_ = [_contig(w.detach(), f32, n) for w, n in ((attn_norm_w, "attn_norm_w"), (char_norm_w, "char_norm_w"), (wq, "wq"), (wk, "wk"), (wv, "wv"), (wo, "wo"))]
    if ws_[0].shape != (D,) or ws_[1].shape != (D,) or any(w.shape != (hdim, D) for w in ws_[2:5]) or ws_[5].shape != (D, hdim):
        raise ValueError(f"char_swa: weight shapes do not fit dim {D}, heads {n_heads} x {head_dim}")
    lams = [None if l is None else _contig(l.detach().reshape(1), f32, "lambda") for l in (lambda_tok, lambda_char)]
    d = capi.MotCharSwaDesc()
    d.struct_size = C.sizeof(capi.MotCharSwaDesc)
    d.dtype, d.n_rows, d.tokens_per_row = capi.F32, B, T
    d.c_v, d.window, d.n_heads, d.head_dim, d.dim = cid.shape[2], int(window), int(n_heads), int(head_dim), D
    d.version = _SWA_VERSIONS[version]
    mm_bf16 = (bf and D % 8 == 0 and hdim % 8 == 0) if matmul is None else matmul == "bf16"
    d.matmul_dtype = capi.BF16 if mm_bf16 else capi.F32
    d.tokens, d.char_ids = capi.ptr(tok), capi.ptr(cid)
    d.tok_table, d.tok_rows, d.char_table, d.char_rows = capi.ptr(tt), tt.shape[0], capi.ptr(ct), ct.shape[0]
    d.norm_eps = float(norm_eps)
    d.attn_norm_w, d.char_norm_w, d.wq, d.wk, d.wv, d.wo = (capi.ptr(w) for w in ws_)
    d.lambda_tok, d.lambda_char = capi.ptr(lams[0]), capi.ptr(lams[1])
    d.io_dtype = capi.BF16 if (bf and mm_bf16) else capi.F32   # bf16 tables: the last product writes the bf16 result itself
    out = torch.empty((B, T, D), dtype=torch.bfloat16 if d.io_dtype == capi.BF16 else f32, device=dev)
    d.out = capi.ptr(out)
    if kv_cache is not None:
        n = 2 * ct.shape[0] * hdim
        if kv_cache.get("buf") is None or kv_cache["buf"].numel() != n or kv_cache["buf"].device != dev:
            kv_cache["buf"], kv_cache["key"] = torch.empty(n, dtype=f32, device=dev), None
        d.kv_tables, d.kv_tables_ready = capi.ptr(kv_cache["buf"]), int(kv_cache.get("key") == kv_key + (str(dev),))
        kv_cache["key"] = kv_key + (str(dev),)
    _launch(dev, d, capi.lib.mot_char_swa_fwd, ws_bytes=capi.lib.mot_char_swa_workspace_bytes)
    return out.to(torch.bfloat16) if bf else out


class CharSwaState(NamedTuple):
    """The device-side state of char_swa_step: ring (B, window, c_v) int32, the characters of source position s in slot
    s % window; pos (B,) int64, the tokens of each row seen so far.  Both are updated in place by every step."""
    ring: torch.Tensor
    pos: torch.Tensor


def char_swa_state(char_ids: torch.Tensor | None = None, *, n_rows: int | None = None, window: int = 8, c_v: int = 8,
                   device=None) -> CharSwaState:
    """The state after a prompt whose character matrix is char_ids (B, T, c_v), or the empty state of n_rows rows (char_ids None).
    Plain torch indexing on `device` (default: char_ids' device): no library call, so it also runs on the host."""
    window = int(window)
    if char_ids is None:
        if n_rows is None:
            raise ValueError("char_swa_state: give char_ids (B, T, c_v) or n_rows")
        return CharSwaState(torch.zeros((int(n_rows), window, int(c_v)), dtype=torch.int32, device=device),
                            torch.zeros(int(n_rows), dtype=torch.int64, device=device))
    if char_ids.ndim == 2:
        char_ids = char_ids[None]
    if char_ids.ndim != 3 or (n_rows is not None and char_ids.shape[0] != n_rows):
        raise ValueError(f"char_swa_state: char_ids must be (B, T, c_v), got {tuple(char_ids.shape)}")
    dev = char_ids.device if device is None else torch.device(device)
    B, T, cv = char_ids.shape
    ring = torch.zeros((B, window, cv), dtype=torch.int32, device=dev)
    src = torch.arange(max(0, T - window), T, device=dev)          # the last `window` positions: one per slot
    ring[:, src % window] = char_ids.to(dev)[:, src].to(torch.int32)
    return CharSwaState(ring, torch.full((B,), T, dtype=torch.int64, device=dev))


@torch.compiler.disable
@torch.no_grad()
def char_swa_step(tokens: torch.Tensor, state: CharSwaState, tok_table: torch.Tensor, char_table: torch.Tensor, *,
                  tok_chars: torch.Tensor | None = None, char_ids_new: torch.Tensor | None = None,
                  attn_norm_w: torch.Tensor, char_norm_w: torch.Tensor, wq: torch.Tensor, wk: torch.Tensor, wv: torch.Tensor, wo: torch.Tensor,
                  n_heads: int, head_dim: int, window: int = 8, norm_eps: float = 1e-5, version: str = "two_residual",
                  lambda_tok: torch.Tensor | None = None, lambda_char: torch.Tensor | None = None, matmul: str | None = None,
                  kv_cache: dict) -> torch.Tensor:
    """One decode step of the character mixer (mot_char_swa_step): tokens (B,) int64 on the device (NextToken.token is read in
    place), B <= 16 -> (B, dim), row t = state.pos of what char_swa computes for each sequence; state is updated in place.  The new
    tokens' characters come from tok_chars (vocab, c_v) int32 (CharTokenizer.token_char_table) or from char_ids_new (B, c_v).
    `kv_cache` must hold the key / value tables a char_swa call (the prefill) built for these parameters.  bf16 tables: the tables,
    wq and wo are read in place as bf16, the result is bf16, the rounding points are char_swa's.  Nothing is read on the host, so
    the call captures into a hipGraph.  Forms no gradients."""
    if matmul not in (None, "fp32", "bf16"):
        raise ValueError(f"char_swa_step: matmul must be None, 'fp32' or 'bf16' (got {matmul!r})")
    bf = tok_table.dtype == torch.bfloat16
    if (bf and matmul == "fp32") or (not bf and matmul == "bf16"):
        raise NotImplementedError("char_swa_step: the step runs in the tables' dtype (bf16 tables on the bf16 path, fp32 tables in fp32); "
                                  "use char_swa for the other combinations")
    params = (tok_table, char_table, attn_norm_w, char_norm_w, wq, wk, wv, wo, lambda_tok, lambda_char)
    dev = capi.require_device(tokens, state.ring, state.pos, tok_chars, char_ids_new, *params)
    tdt = torch.bfloat16 if bf else torch.float32
    if (tok_chars is None) == (char_ids_new is None):
        raise ValueError("char_swa_step: give exactly one of tok_chars and char_ids_new")
    kv_key = tuple((t.data_ptr(), t._version) for t in (char_table, char_norm_w, wk, wv)) + (float(norm_eps), str(char_table.dtype), str(dev))
    D, hdim, char_rows = tok_table.shape[1], int(n_heads) * int(head_dim), char_table.shape[0]
    buf = None if kv_cache is None else kv_cache.get("buf")
    if buf is None or kv_cache.get("key") != kv_key or buf.numel() != 2 * char_rows * hdim or buf.device != dev:
        raise RuntimeError("char_swa_step: kv_cache holds no current key / value tables for these parameters; run char_swa (the prefill) "
                           "with this kv_cache first")
    ring, pos = state
    if ring.dtype != torch.int32 or pos.dtype != torch.int64 or ring.ndim != 3 or not ring.is_contiguous() or not pos.is_contiguous() \
            or pos.shape != (ring.shape[0],) or ring.shape[1] != int(window):
        raise ValueError("char_swa_step: state must be char_swa_state's (ring (B, window, c_v) int32, pos (B,) int64), contiguous")
    B, _, c_v = ring.shape
    if tokens.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"char_swa_step: tokens must be int64 (NextToken.token) or int32, got {tokens.dtype}")
    tok = _contig(tokens.detach().reshape(-1).to(torch.int64), torch.int64, "tokens")
    if tok.numel() != B:
        raise ValueError(f"char_swa_step: {tok.numel()} tokens for a state of {B} rows")
    if char_table.dtype != tdt or char_table.shape[1] != D:
        raise TypeError("char_swa_step: char_table must have tok_table's dtype and number of columns")
    tt, ct = _contig(tok_table.detach(), tdt, "tok_table"), _contig(char_table.detach(), tdt, "char_table")
    wq_, wo_ = _contig(wq.detach(), tdt, "wq"), _contig(wo.detach(), tdt, "wo")
    if attn_norm_w.shape != (D,) or wq_.shape != (hdim, D) or wo_.shape != (D, hdim):
        raise ValueError(f"char_swa_step: weight shapes do not fit dim {D}, heads {n_heads} x {head_dim}")
    # the norm weight and the lambdas are fp32 device memory in both modes: with bf16 parameters their widened copies are kept in
    # kv_cache beside char_swa's, while the originals are unchanged
    wide_cache = kv_cache.setdefault("widened", {})

    def f32_of(t, shape):
        if t is None:
            return None
        if t.dtype == torch.float32:
            return _contig(t.detach().reshape(shape), torch.float32, "parameter")
        key = (t.data_ptr(), t._version, tuple(t.shape), str(t.dtype))
        hit = wide_cache.get(id(t))
        if hit is None or hit[0] != key:
            hit = wide_cache[id(t)] = (key, t.detach().to(torch.bfloat16).float(), t)
        return hit[1].reshape(shape)
    anw, lt, lc = f32_of(attn_norm_w, (D,)), f32_of(lambda_tok, (1,)), f32_of(lambda_char, (1,))
    d = capi.MotCharSwaStepDesc()
    d.struct_size = C.sizeof(capi.MotCharSwaStepDesc)
    d.dtype, d.n_rows, d.c_v, d.window, d.n_heads, d.head_dim, d.dim = capi.dtype_code(tdt), B, c_v, int(window), int(n_heads), int(head_dim), D
    d.version, d.char_rows, d.tok_rows, d.norm_eps = _SWA_VERSIONS[version], char_rows, tt.shape[0], float(norm_eps)
    keep = [tok]
    if tok_chars is not None:
        if tok_chars.dtype != torch.int32 or tok_chars.shape != (tt.shape[0], c_v) or not tok_chars.is_contiguous():
            raise ValueError(f"char_swa_step: tok_chars must be the contiguous int32 ({tt.shape[0]}, {c_v}) table of token_char_table")
        d.tok_chars = capi.ptr(tok_chars)
    else:
        cn = _contig(char_ids_new.detach().reshape(-1, c_v), torch.int64, "char_ids_new")
        if cn.shape[0] != B:
            raise ValueError(f"char_swa_step: char_ids_new must be ({B}, {c_v})")
        keep.append(cn)
        d.char_ids_new = capi.ptr(cn)
    d.tokens, d.tok_table, d.char_table, d.attn_norm_w, d.wq, d.wo = capi.ptr(tok), capi.ptr(tt), capi.ptr(ct), capi.ptr(anw), capi.ptr(wq_), capi.ptr(wo_)
    d.lambda_tok, d.lambda_char, d.kv_tables, d.ring, d.pos = capi.ptr(lt), capi.ptr(lc), capi.ptr(buf), capi.ptr(ring), capi.ptr(pos)
    out = torch.empty((B, D), dtype=tdt, device=dev)
    d.out = capi.ptr(out)
    _launch(dev, d, capi.lib.mot_char_swa_step, ws_bytes=capi.lib.mot_char_swa_step_workspace_bytes)
    return out


@torch.compiler.disable
@torch.no_grad()
def char_ffn_step(h: torch.Tensor, norm_w: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor, w3: torch.Tensor, *, norm_eps: float = 1e-5,
                  cache: dict | None = None) -> torch.Tensor:
    """The feed-forward that closes the character mixer's block on the rows of a decode step (mot_ffn_step): h (B, dim), B <= 16,
    char_swa_step's result -> ``h + w2(silu(w1 n) * w3 n)``, ``n = RMSNorm(h) * norm_w``; w1 and w3 (inter, dim), w2 (dim, inter),
    FeedForward's weights, used in place.  h and the three matrices share one dtype, fp32 or bf16 (then the rounding points are
    those of the module in a bf16 cast); norm_w is fp32 device memory in the call: the widened copy of a bf16 norm weight is kept
    in `cache` (as char_swa_step keeps its own in kv_cache) while the weight is unchanged.  Nothing is read on the host, so the call
    captures into a hipGraph.  Forms no gradients."""
    dev = capi.require_device(h, norm_w, w1, w2, w3)
    tdt = h.dtype
    capi.dtype_code(tdt)
    if h.ndim != 2:
        raise ValueError(f"char_ffn_step: h must be (B, dim), got {tuple(h.shape)}")
    B, D = h.shape
    if B > 16:
        raise NotImplementedError(f"char_ffn_step: {B} rows, the step is built for at most 16: use FeedForward (h + feed_forward(ffn_norm(h)))")
    h_ = _contig(h.detach(), tdt, "h")
    w1_, w2_, w3_ = _contig(w1.detach(), tdt, "w1"), _contig(w2.detach(), tdt, "w2"), _contig(w3.detach(), tdt, "w3")
    inter = w1_.shape[0]
    if norm_w.shape != (D,) or w1_.shape != (inter, D) or w3_.shape != (inter, D) or w2_.shape != (D, inter):
        raise ValueError(f"char_ffn_step: weight shapes do not fit h {tuple(h.shape)}: norm_w ({D},), w1 and w3 (inter, {D}), w2 ({D}, inter)")
    if norm_w.dtype == torch.float32:
        nw = _contig(norm_w.detach(), torch.float32, "norm_w")
    else:
        key = (norm_w.data_ptr(), norm_w._version, str(norm_w.dtype), str(dev))
        hit = None if cache is None else cache.get("norm_w")
        if hit is None or hit[0] != key:
            hit = (key, norm_w.detach().to(torch.bfloat16).float().contiguous(), norm_w)
            if cache is not None:
                cache["norm_w"] = hit
        nw = hit[1]
    d = capi.MotFfnStepDesc()
    d.struct_size = C.sizeof(capi.MotFfnStepDesc)
    d.dtype, d.n_rows, d.dim, d.inter, d.norm_eps = capi.dtype_code(tdt), B, D, inter, float(norm_eps)
    d.h, d.norm_w, d.w1, d.w3, d.w2 = capi.ptr(h_), capi.ptr(nw), capi.ptr(w1_), capi.ptr(w3_), capi.ptr(w2_)
    out = torch.empty((B, D), dtype=tdt, device=dev)
    d.out = capi.ptr(out)
    _launch(dev, d, capi.lib.mot_ffn_step, ws_bytes=capi.lib.mot_ffn_step_workspace_bytes)
    return out


# ----------------------------------------------------------------------------------------------
# byte output head: mixout (identity layers) + norm + lm_head + softcap + cross-entropy, train_gpt.py:618-623
# ----------------------------------------------------------------------------------------------
_HEAD_METHODS = {"copy": capi.HEAD_COPY, "split": capi.HEAD_SPLIT}


def _byte_head_desc(x, w, targets, method, bpt, n_layer_out, row_stats, loss):
    if method not in _HEAD_METHODS:
        raise ValueError(f"byte_head_loss: method must be 'copy' or 'split', got {method!r}")
    dev = capi.require_device(x, w, targets)
    d = capi.MotByteHeadDesc()
    d.struct_size = C.sizeof(capi.MotByteHeadDesc)
    d.method, d.dtype, d.bpt = _HEAD_METHODS[method], capi.dtype_code(x.dtype), int(bpt)
    d.n_tokens, d.model_dim, d.n_layer_out, d.vocab, d.eps = x.shape[0], x.shape[1], int(n_layer_out), w.shape[0], 0.0
    d.x, d.weight, d.targets, d.loss, d.row_stats = capi.ptr(x), capi.ptr(w), capi.ptr(targets), capi.ptr(loss), capi.ptr(row_stats)
    return d, dev


def _head_operands(fn, x, weight, targets, per_row, rows_as):
    """What the two output heads do to their operands once their own checks have passed: x flat and detached, the weight cast once
    to x's dtype as CastedLinear does (train_gpt.py:185-186, lm_head_w.bfloat16()), the int64 targets flat, per_row to a row of x."""
    x2 = _contig(x.detach().reshape(-1, x.shape[-1]), x.dtype, "x")
    w = _contig(weight.detach().to(x2.dtype), x2.dtype, "weight")
    t = _contig(targets.reshape(-1), torch.int64, "targets")
    if t.numel() != x2.shape[0] * per_row:
        raise ValueError(f"{fn}: {t.numel()} targets for {x2.shape[0]} {rows_as}")
    return x2, w, t


def _byte_head_operands(x, weight, targets, bpt):
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"byte_head_loss: x must be float32 or bfloat16, got {x.dtype}")
    x2, w, t = _head_operands("byte_head_loss", x, weight, targets, bpt, f"tokens x {bpt} bytes")   # non-int64 targets are refused there
    if w.ndim != 2:
        raise ValueError("byte_head_loss: weight must be (vocab, in_features)")
    return x2, w, t


class _ByteHeadFn(torch.autograd.Function):
    """forward = mot_byte_head_fwd (the loss and the per-row lse / norm factor), backward = mot_byte_head_bwd (dx, fp32 dW)."""

    @staticmethod
    def forward(ctx, x, weight, targets, method, bpt, n_layer_out):
        x2, w, t = _byte_head_operands(x, weight, targets, bpt)
        rows = x2.shape[0] * (bpt if method == "split" else 1)
        row_stats = torch.empty(2 * rows, dtype=torch.float32, device=x2.device)
        loss = torch.empty((), dtype=torch.float32, device=x2.device)
        d, dev = _byte_head_desc(x2, w, t, method, bpt, n_layer_out, row_stats, loss)
        _launch(dev, d, capi.lib.mot_byte_head_fwd, ws_bytes=capi.lib.mot_byte_head_workspace_bytes)
        ctx.save_for_backward(x2, w, t, row_stats)
        ctx.cfg = (method, bpt, n_layer_out, x.shape, weight.dtype)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        x2, w, t, row_stats = ctx.saved_tensors
        method, bpt, n_layer_out, xshape, wdtype = ctx.cfg
        d, dev = _byte_head_desc(x2, w, t, method, bpt, n_layer_out, row_stats, None)
        go = _contig(grad_loss.detach().reshape(()).float(), torch.float32, "grad_loss")
        dx = torch.empty_like(x2)
        dw = torch.empty(w.shape, dtype=torch.float32, device=dev)
        _launch(dev, d, capi.lib.mot_byte_head_bwd, capi.ptr(go), capi.ptr(dx), capi.ptr(dw), ws_bytes=capi.lib.mot_byte_head_workspace_bytes)
        return dx.reshape(xshape), dw.to(wdtype), None, None, None, None


def _byte_head_step_call(x2, w, t, bpt, n_layer_out, dx, dw):
    """One mot_byte_head_step: the loss, and the gradients for grad_loss = 1 into dx / dw where given."""
    loss = torch.empty((), dtype=torch.float32, device=x2.device)
    d, dev = _byte_head_desc(x2, w, t, "split", bpt, n_layer_out, None, loss)
    _launch(dev, d, capi.lib.mot_byte_head_step, capi.ptr(dx), capi.ptr(dw), ws_bytes=capi.lib.mot_byte_head_step_workspace_bytes)
    return loss


def _byte_head_step_operands(x, weight, targets, method, bpt, n_layer_out):
    """The operands of the one-call form.  What the call does not build (copy mode, a row width or dtype outside its limits) is
    refused by the library itself, from the shapes alone and before the device check: NotImplementedError with its message."""
    if method not in _HEAD_METHODS:
        raise ValueError(f"byte_head_loss: method must be 'copy' or 'split', got {method!r}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"byte_head_loss: x must be float32 or bfloat16, got {x.dtype}")
    if weight.ndim != 2:
        raise ValueError("byte_head_loss: weight must be (vocab, in_features)")
    d = capi.MotByteHeadDesc()
    d.struct_size = C.sizeof(capi.MotByteHeadDesc)
    d.method, d.dtype, d.bpt = _HEAD_METHODS[method], capi.dtype_code(x.dtype), int(bpt)
    d.n_tokens, d.model_dim, d.n_layer_out, d.vocab = x.numel() // max(x.shape[-1], 1), x.shape[-1], int(n_layer_out), weight.shape[0]
    rc = capi.lib.mot_byte_head_step(C.byref(d), None, None, None)   # no pointers: the shape checks come first, nothing is launched
    if rc in (capi.MOT_EUNSUPPORTED, capi.MOT_ESHAPE):
        capi.check(rc)
    capi.require_device(x, weight, targets)
    return _byte_head_operands(x, weight, targets, bpt)


def _scale_head_grads(ctx, grad_loss, need_x=True, need_w=True):
    """The backward of the head Functions whose forward formed dx and the fp32 dW for grad_loss = 1 and saved them (either may be
    None) with cfg = (x.shape, weight.dtype, ...): both times the incoming grad_loss, on the device and out of place."""
    dx, dw = ctx.saved_tensors
    xshape, wdtype = ctx.cfg[:2]
    go = grad_loss.detach().reshape(1, 1).float()
    gx = gw = None
    if need_x and dx is not None:   # one elementwise pass: fp32 factor, fp32 product, one rounding on store, no fp32 copy of dx
        gx = torch.mul(dx, go, out=torch.empty_like(dx)).reshape(xshape)
    if need_w and dw is not None:
        gw = torch.mul(dw, go, out=torch.empty(dw.shape, dtype=wdtype, device=dw.device))
    return gx, gw


class _ByteHeadStepFn(torch.autograd.Function):
    """forward = one mot_byte_head_step that also forms dx and the fp32 dW for grad_loss = 1; backward multiplies them by the incoming
    grad_loss on the device, out of place (a retained graph runs backward again on the same saved gradients)."""

    @staticmethod
    def forward(ctx, x, weight, targets, method, bpt, n_layer_out):
        x2, w, t = _byte_head_step_operands(x, weight, targets, method, bpt, n_layer_out)
        dx = torch.empty_like(x2)
        dw = torch.empty(w.shape, dtype=torch.float32, device=x2.device)
        loss = _byte_head_step_call(x2, w, t, bpt, n_layer_out, dx, dw)
        ctx.save_for_backward(dx, dw)
        ctx.cfg = (x.shape, weight.dtype, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        return _scale_head_grads(ctx, grad_loss, *ctx.cfg[2:]) + (None,) * 4


@torch.compiler.disable
def byte_head_loss(x: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor, *, method: str, bytes_per_token: int,
                   n_layer_out: int = 0, one_call: bool = False) -> torch.Tensor:
    """The byte output head of a mixout run with identity layers (use_byte_self_attn off), train_gpt.py:618-623:
    h = repeat (copy) or rearrange (split) of x into byte rows; h = h + norm(h) n_layer_out times; logits = norm(h) @ weight.T;
    z = 30 sigmoid(logits.float() / 7.5); returns cross_entropy(z, targets) (mean over all n_tokens * bytes_per_token targets) as an
    fp32 scalar.  x (..., model_dim) float32 or bfloat16; weight (512, model_dim or model_dim / bpt), cast to x's dtype as CastedLinear
    does; targets int64 (..., T * bpt).  Differentiable in x and weight (the weight's gradient in the weight's dtype).
    A target outside [0, 512) raises the status bit that check_status() reports; its term is left out of the sum.
    one_call=True takes the split-mode step on one fused kernel (mot_byte_head_step): with grad mode on, the one call forms the loss,
    dx and the fp32 dW, and backward only scales them by the incoming gradient; under no_grad, or with neither input requiring a
    gradient, it is the loss alone, with the same bits.  It is built for method="split" with a row width model_dim / bytes_per_token
    that is a multiple of 16 and at most 128 in bfloat16, 64 in float32; anything else raises NotImplementedError here, with the
    library's message (there is no fallback to the two-call path)."""
    if one_call:
        bpt, L = int(bytes_per_token), int(n_layer_out)
        if not torch.is_grad_enabled() or not (x.requires_grad or weight.requires_grad):
            x2, w, t = _byte_head_step_operands(x, weight, targets, method, bpt, L)
            return _byte_head_step_call(x2, w, t, bpt, L, None, None)
        return _ByteHeadStepFn.apply(x, weight, targets, method, bpt, L)
    return _ByteHeadFn.apply(x, weight, targets, method, int(bytes_per_token), int(n_layer_out))


# ----------------------------------------------------------------------------------------------
# token-level output head: norm + lm_head + softcap + cross-entropy, train_gpt.py:619-623 (noop mixout), runs/71_*.py:331-334
# ----------------------------------------------------------------------------------------------
_SOFTCAPS = {"sigmoid30": capi.SOFTCAP_SIGMOID30, "rsqrt15": capi.SOFTCAP_RSQRT15}


def _token_head_desc(x2, w, t, softcap, norm_in, chunk_rows):
    dev = capi.require_device(x2, w, t)
    d = capi.MotTokenHeadDesc()
    d.struct_size = C.sizeof(capi.MotTokenHeadDesc)
    d.dtype, d.softcap, d.norm_in, d.chunk_rows = capi.dtype_code(x2.dtype), _SOFTCAPS[softcap], int(bool(norm_in)), int(chunk_rows or 0)
    d.n_rows, d.model_dim, d.vocab, d.eps = x2.shape[0], x2.shape[1], w.shape[0], 0.0
    d.x, d.weight, d.targets = capi.ptr(x2), capi.ptr(w), capi.ptr(t)
    return d, dev


def _token_head_call(x2, w, t, softcap, norm_in, chunk_rows, dx, dw):
    """One mot_token_head_fwd: the loss, and the gradients for grad_loss = 1 into dx / dw where given."""
    d, dev = _token_head_desc(x2, w, t, softcap, norm_in, chunk_rows)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    d.loss, d.dx, d.dW = capi.ptr(loss), capi.ptr(dx), capi.ptr(dw)
    _launch(dev, d, capi.lib.mot_token_head_fwd, ws_bytes=capi.lib.mot_token_head_workspace_bytes)
    return loss


def _wide_head_operands(fn, x, weight, targets):
    """The operand checks of the token-level and the plain head, then x as rows, the weight in x's dtype and int64 targets; `fn`,
    the public function's name, starts the messages."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{fn}: x must be float32 or bfloat16, got {x.dtype}")
    if weight.ndim != 2 or weight.shape[1] != x.shape[-1]:
        raise ValueError(f"{fn}: weight must be (vocab, {x.shape[-1]}), got {tuple(weight.shape)}")
    if targets.dtype not in (torch.int64, torch.int32):
        raise TypeError(f"{fn}: targets must be int64 or int32, got {targets.dtype}")
    capi.require_device(x, weight, targets)
    return _head_operands(fn, x, weight, targets.to(torch.int64), 1, "rows")


def _token_head_operands(x, weight, targets, softcap):
    if softcap not in _SOFTCAPS:
        raise ValueError(f"token_head_loss: softcap must be 'sigmoid30' or 'rsqrt15', got {softcap!r}")
    return _wide_head_operands("token_head_loss", x, weight, targets)


class _TokenHeadFn(torch.autograd.Function):
    """forward = one mot_token_head_fwd that also forms dx and the fp32 dW for grad_loss = 1; backward multiplies them by the incoming
    grad_loss on the device, out of place (a retained graph runs backward again on the same saved gradients)."""

    @staticmethod
    def forward(ctx, x, weight, targets, softcap, norm_in, chunk_rows):
        x2, w, t = _token_head_operands(x, weight, targets, softcap)
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = torch.empty_like(x2) if need_x else None
        dw = torch.empty(w.shape, dtype=torch.float32, device=x2.device) if need_w else None
        loss = _token_head_call(x2, w, t, softcap, norm_in, chunk_rows, dx, dw)
        ctx.save_for_backward(dx, dw)
        ctx.cfg = (x.shape, weight.dtype)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        return _scale_head_grads(ctx, grad_loss) + (None,) * 4


@torch.compiler.disable
def token_head_loss(x: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor, *, softcap: str = "sigmoid30", norm_in: bool = True,
                    chunk_rows: int | None = None) -> torch.Tensor:
    """The token-level output head, fused: cross_entropy(cap(F.linear(norm(x), weight).float()), targets) as an fp32 scalar, with
    cap = 30 sigmoid(l / 7.5) ("sigmoid30", scaled-pre-train/train_gpt.py:619-623 with byte_mixout_method "noop") or
    15 l rsqrt(l^2 + 225) ("rsqrt15", modded-nanogpt/runs/71_*.py:331-334); norm_in=False takes x as already normed.
    x (..., model_dim) float32 or bfloat16; weight (vocab, model_dim), cast once to x's dtype as CastedLinear does; targets int64 or
    int32 (...).  No logits tensor of rows x vocab exists: the rows run in chunks (chunk_rows rows, a multiple of 32; None: the
    library's choice).  Differentiable in x and weight (the weight's gradient in the weight's dtype, summed in fp32): with grad mode
    on, the one call forms both gradients beside the loss; under no_grad it is the loss alone, with the same bits.
    A target outside [0, vocab) raises the status bit that check_status() reports; its term is left out of the sum."""
    if not torch.is_grad_enabled() or not (x.requires_grad or weight.requires_grad):
        x2, w, t = _token_head_operands(x, weight, targets, softcap)
        return _token_head_call(x2, w, t, softcap, norm_in, chunk_rows, None, None)
    return _TokenHeadFn.apply(x, weight, targets, softcap, bool(norm_in), chunk_rows)


# ----------------------------------------------------------------------------------------------
# evaluation form of the two heads: the no-grad loss pass that also writes per-row loss, top-1 prediction and target rank
# ----------------------------------------------------------------------------------------------
class HeadEval(NamedTuple):
    """What token_head_eval / byte_head_eval return.  A row is a token (token-level head) or a byte position (byte head), in the
    targets' shape.  loss: the fp32 scalar of the loss call, the same bits; row_loss fp32: lse(z) - z[target], 0 for a target out of
    range; pred int32: the class of the largest logit, the lowest on ties (-1 for a dropped row of plain_head_eval with max_kept: its
    logits are never formed); rank int32: the number of classes whose logit is strictly
    above the target's, -1 for a target out of range; counts int64 on the device: [rows with a target in range, those with
    pred == target], and for the byte head a third, the tokens all of whose byte predictions equal their targets."""
    loss: torch.Tensor
    row_loss: torch.Tensor
    pred: torch.Tensor
    rank: torch.Tensor
    counts: torch.Tensor


def _head_eval_call(dev, d, fn, ws_bytes, shape, n_counts, *pre):
    """The tail of the evaluation calls: the outputs in the targets' shape, the out struct, the launch (`pre`: what the call takes
    between the descriptor and the out struct)."""
    n = math.prod(shape)
    row_loss = torch.empty(n, dtype=torch.float32, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    rank = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(n_counts, dtype=torch.int64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    d.loss = capi.ptr(loss)
    o = capi.MotHeadEvalOut()
    o.struct_size = C.sizeof(capi.MotHeadEvalOut)
    o.row_loss, o.pred, o.rank, o.counts = capi.ptr(row_loss), capi.ptr(pred), capi.ptr(rank), capi.ptr(counts)
    _launch(dev, d, fn, *pre, C.byref(o), ws_bytes=ws_bytes)
    return HeadEval(loss, row_loss.reshape(shape), pred.reshape(shape), rank.reshape(shape), counts)


@torch.compiler.disable
@torch.no_grad()
def token_head_eval(x: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor, *, softcap: str = "sigmoid30", norm_in: bool = True,
                    chunk_rows: int | None = None) -> HeadEval:
    """The token-level head for evaluation: the pass of token_head_loss under no_grad over the same chunks, which also writes every
    token's loss, top-1 prediction and target rank (HeadEval) without any tensor of rows x vocab.  Arguments as token_head_loss;
    HeadEval.loss has the bits of that call.  pred and rank are taken on the stored products x W^T (bf16 with bfloat16 x), in front of
    the norm's positive factor and the increasing softcap: rank < k is top-k accuracy.  Forms no gradients in any grad mode.
    A target outside [0, vocab) raises the status bit that check_status() reports and is left out of loss and counts."""
    x2, w, t = _token_head_operands(x, weight, targets, softcap)   # held until the launch: the descriptor has only their addresses
    d, dev = _token_head_desc(x2, w, t, softcap, norm_in, chunk_rows)
    return _head_eval_call(dev, d, capi.lib.mot_token_head_eval, capi.lib.mot_token_head_workspace_bytes, targets.shape, 2)


@torch.compiler.disable
@torch.no_grad()
def byte_head_eval(x: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor, *, method: str, bytes_per_token: int,
                   n_layer_out: int = 0) -> HeadEval:
    """The byte head for evaluation: the forward of byte_head_loss over the same chunks, which also writes every byte position's
    loss, top-1 prediction and target rank (HeadEval, in the targets' shape) without any tensor of positions x 512.  Arguments as
    byte_head_loss; HeadEval.loss has the bits of that call under no_grad.  In copy mode the head computes one row per token: pred
    is that row's prediction at each of the token's positions, row_loss and rank are each position's own.  counts[2] is the number of
    tokens with every byte right: the whole-token accuracy a token-level model reports as counts[1].  Forms no gradients."""
    bpt = int(bytes_per_token)
    x2, w, t = _byte_head_operands(x, weight, targets, bpt)
    d, dev = _byte_head_desc(x2, w, t, method, bpt, n_layer_out, None, None)
    return _head_eval_call(dev, d, capi.lib.mot_byte_head_eval, capi.lib.mot_byte_head_workspace_bytes, targets.shape, 3)


# ----------------------------------------------------------------------------------------------
# plain cross-entropy head: lm_head + cross_entropy without a softcap, with ignore_index and the mean over the kept targets,
# mathblations/model.py:337-338 + main.py:294-303 (evaluation :164-187), inference/inference.py:349-359
# ----------------------------------------------------------------------------------------------
def _plain_head_desc(x2, w, t, norm_in, ignore_index, chunk_rows, group_rows=0):
    dev = capi.require_device(x2, w, t)
    d = capi.MotPlainHeadDesc()
    d.struct_size = C.sizeof(capi.MotPlainHeadDesc)
    d.dtype, d.norm_in, d.chunk_rows, d.group_rows = capi.dtype_code(x2.dtype), int(bool(norm_in)), int(chunk_rows or 0), int(group_rows or 0)
    d.n_rows, d.model_dim, d.vocab, d.eps, d.ignore_index = x2.shape[0], x2.shape[1], w.shape[0], 0.0, int(ignore_index)
    d.x, d.weight, d.targets = capi.ptr(x2), capi.ptr(w), capi.ptr(t)
    return d, dev


def _max_kept_arg(fn, max_kept):
    """max_kept of the plain head's calls: None (every row's logits are formed) or a positive int, checked before anything else."""
    if max_kept is None:
        return None
    if isinstance(max_kept, bool) or not isinstance(max_kept, numbers.Integral) or max_kept <= 0:
        raise ValueError(f"{fn}: max_kept must be None or a positive int (a host bound on the kept rows), got {max_kept!r}")
    return int(max_kept)


def _plain_head_compact(max_kept):
    """The MotPlainHeadCompact of a call with max_kept, and the workspace query bound to it."""
    c = capi.MotPlainHeadCompact()
    c.struct_size, c.reserved, c.max_kept = C.sizeof(capi.MotPlainHeadCompact), 0, max_kept
    return c, lambda p: capi.lib.mot_plain_head_compact_workspace_bytes(p, C.byref(c))


def _plain_head_call(x2, w, t, norm_in, ignore_index, chunk_rows, dx, dw, max_kept=None):
    """One mot_plain_head_fwd (max_kept None) or mot_plain_head_compact_fwd: the loss, and the gradients for grad_loss = 1 into
    dx / dw where given."""
    d, dev = _plain_head_desc(x2, w, t, norm_in, ignore_index, chunk_rows)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    d.loss, d.dx, d.dW = capi.ptr(loss), capi.ptr(dx), capi.ptr(dw)
    if max_kept is None:
        _launch(dev, d, capi.lib.mot_plain_head_fwd, ws_bytes=capi.lib.mot_plain_head_workspace_bytes)
    else:
        c, ws_bytes = _plain_head_compact(max_kept)
        _launch(dev, d, capi.lib.mot_plain_head_compact_fwd, C.byref(c), ws_bytes=ws_bytes)
    return loss


class _PlainHeadFn(torch.autograd.Function):
    """forward = one mot_plain_head_fwd (mot_plain_head_compact_fwd with max_kept) that also forms dx and the fp32 dW for
    grad_loss = 1; backward multiplies them by the incoming grad_loss on the device, out of place (a retained graph runs backward
    again on the same saved gradients)."""

    @staticmethod
    def forward(ctx, x, weight, targets, norm_in, ignore_index, chunk_rows, max_kept=None):
        x2, w, t = _wide_head_operands("plain_head_loss", x, weight, targets)
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = torch.empty_like(x2) if need_x else None
        dw = torch.empty(w.shape, dtype=torch.float32, device=x2.device) if need_w else None
        loss = _plain_head_call(x2, w, t, norm_in, ignore_index, chunk_rows, dx, dw, max_kept)
        ctx.save_for_backward(dx, dw)
        ctx.cfg = (x.shape, weight.dtype)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        return _scale_head_grads(ctx, grad_loss) + (None,) * 5


@torch.compiler.disable
def plain_head_loss(x: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor, *, norm_in: bool = True, ignore_index: int = -100,
                    chunk_rows: int | None = None, max_kept: int | None = None) -> torch.Tensor:
    """The plain cross-entropy head, fused: F.cross_entropy(F.linear(norm(x), weight).float(), targets, ignore_index=ignore_index)
    as an fp32 scalar, with no softcap and the mean over the kept targets: mathblations/model.py:337-338 with main.py:294-303
    (norm_in=True, the scored window marked with window_targets) and inference/inference.py:349-359 (norm_in=False, the shift done by
    the caller).  x (..., model_dim) float32 or bfloat16; weight (vocab, model_dim), cast once to x's dtype; targets int64 or int32
    (...).  No logits tensor of rows x vocab exists: the rows run in chunks (chunk_rows rows, a multiple of 32; None: the library's
    choice).  Differentiable in x and weight (the weight's gradient in the weight's dtype, summed in fp32): with grad mode on, the
    one call forms both gradients beside the loss; under no_grad it is the loss alone, with the same bits.
    A target equal to ignore_index drops its row; any other target outside [0, vocab) drops it too and raises the status bit that
    check_status() reports.  The number of kept targets is counted on the device (the call captures into a hipGraph); with none kept
    the loss is NaN, as torch's, and the gradients are exactly zero.
    max_kept (None: every row's logits are formed, kept or not): a host bound on the number of kept targets, e.g.
    window_kept_bound(ranges, T) or the label mask's count.  The kept rows are then compacted on the device behind
    cap = min(max_kept, rows) and the products, the row pass and the chunks (chunk_rows clipped to cap) run over cap slots, so the
    time and the workspace follow the scored positions; whole padding chunks of a loose bound still run, on zero rows.  The loss is
    the same fixed-order sum over the slots (the same bits on every run, not necessarily those of max_kept=None); dropped rows of
    the gradient are +0.  More kept targets than max_kept is a caller error: the loss is NaN, the gradients are exactly zero and
    check_status() reports the kept overflow; the first max_kept rows are never scored alone."""
    max_kept = _max_kept_arg("plain_head_loss", max_kept)
    if not torch.is_grad_enabled() or not (x.requires_grad or weight.requires_grad):
        x2, w, t = _wide_head_operands("plain_head_loss", x, weight, targets)
        return _plain_head_call(x2, w, t, norm_in, ignore_index, chunk_rows, None, None, max_kept)
    return _PlainHeadFn.apply(x, weight, targets, bool(norm_in), int(ignore_index), chunk_rows, max_kept)


@torch.compiler.disable
@torch.no_grad()
def plain_head_eval(x: torch.Tensor, weight: torch.Tensor, targets: torch.Tensor, *, norm_in: bool = True, ignore_index: int = -100,
                    chunk_rows: int | None = None, group_rows: int = 0, max_kept: int | None = None) -> HeadEval:
    """The plain head for evaluation (mathblations/main.py:164-187): the pass of plain_head_loss under no_grad over the same chunks,
    which also writes every row's loss, top-1 prediction and target rank (HeadEval) without any tensor of rows x vocab.
    HeadEval.loss has the bits of plain_head_loss.  A dropped row (target ignore_index or out of range) has row_loss 0 and rank -1;
    its pred is still written.  counts = [kept rows, kept rows with pred == target]; with group_rows > 0 (the sequence length; it
    must divide the rows) a third entry counts the groups of group_rows consecutive rows that have a kept row and whose kept rows are
    all right, full_correct of main.py:183-187.  Forms no gradients in any grad mode.
    max_kept as in plain_head_loss: the kept rows alone are scored.  Kept rows get what max_kept=None writes; a dropped row's logits
    are never formed, so its pred is -1 (row_loss 0 and rank -1 as before).  The counts keep their definition, HeadEval.loss has the
    bits of plain_head_loss(..., max_kept=max_kept) under no_grad."""
    max_kept = _max_kept_arg("plain_head_eval", max_kept)
    x2, w, t = _wide_head_operands("plain_head_loss", x, weight, targets)
    d, dev = _plain_head_desc(x2, w, t, norm_in, ignore_index, chunk_rows, group_rows)
    n_counts = 3 if group_rows else 2
    if max_kept is None:
        return _head_eval_call(dev, d, capi.lib.mot_plain_head_eval, capi.lib.mot_plain_head_workspace_bytes, targets.shape, n_counts)
    c, ws_bytes = _plain_head_compact(max_kept)
    return _head_eval_call(dev, d, capi.lib.mot_plain_head_compact_eval, ws_bytes, targets.shape, n_counts, C.byref(c))


# ----------------------------------------------------------------------------------------------
# the generation step behind the plain head: logits of the last position, top-k / top-p and the draw, inference/inference.py:420-444
# ----------------------------------------------------------------------------------------------
class NextToken(NamedTuple):
    """What next_token returns, in the shape of x without its last dimension.  token int64: the chosen class, -1 for a row with a NaN or
    +inf logit; prob fp32: its probability after the cuts; kept int32: the classes that survive the cuts; top_cls int32 / top_prob fp32
    (..., n_top): the largest filtered probabilities in descending order, -1 / 0 past the kept count (None at n_top = 0); logits fp32
    (..., vocab): the stored logits in front of the temperature (None unless return_logits)."""
    token: torch.Tensor
    prob: torch.Tensor
    kept: torch.Tensor
    top_cls: torch.Tensor | None
    top_prob: torch.Tensor | None
    logits: torch.Tensor | None


def _next_token_rows(x):
    """x (..., model_dim) as rows the library reads in place: a 2-d view whose rows are contiguous, 16-byte aligned and a fixed number
    of elements apart (hidden[:, -1, :] is one), else a contiguous copy.  Returns (rows, stride in elements)."""
    x2 = x.detach()
    if x2.ndim == 1:
        x2 = x2[None]
    elif x2.ndim != 2:
        x2 = x2.reshape(-1, x2.shape[-1])
    n, dim = x2.shape
    e = x2.element_size()
    ok = n == 0 or ((dim == 1 or x2.stride(1) == 1) and x2.data_ptr() % 16 == 0 and (n == 1 or (x2.stride(0) >= dim and x2.stride(0) * e % 16 == 0)))
    if not ok:
        x2 = x2.contiguous()
    return x2, (x2.stride(0) if n > 1 else dim)


@torch.compiler.disable
@torch.no_grad()
def next_token(x: torch.Tensor, weight: torch.Tensor, *, norm_in: bool = False, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0,
               greedy: bool = False, u: torch.Tensor | None = None, n_top: int = 0, return_logits: bool = False) -> NextToken:
    """One generation step, fused (inference/inference.py:420-444): lm_head on the rows of x (the last position's hidden states),
    / temperature, the top-k cut (0 < top_k < vocab), the top-p cut over its survivors (top_p < 1), then argmax (greedy) or the
    inverse-CDF draw with u, one uniform number in [0, 1) per row (None: torch.rand on the device, so the call stays capturable).
    x (..., model_dim) float32 or bfloat16, read in place when its rows are a fixed stride apart; weight (vocab, model_dim), cast to
    x's dtype.  Decisions are taken on the stored logits (bf16 with bfloat16 x).  top-k keeps every class tied with the k-th value;
    top-p keeps a class when the mass of the strictly larger logits is <= top_p and keeps a tie group whole; the draw takes the first
    kept class, in ascending class order, whose running mass exceeds u * (kept mass).  Nothing is read on the host, no sort, no tensor
    beyond the logits.  Forms no gradients in any grad mode."""
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"next_token: x must be float32 or bfloat16, got {x.dtype}")
    if weight.ndim != 2 or weight.shape[1] != x.shape[-1]:
        raise ValueError(f"next_token: weight must be (vocab, {x.shape[-1]}), got {tuple(weight.shape)}")
    dev = capi.require_device(x, weight, u)
    x2, stride = _next_token_rows(x)
    n, shape, vocab, n_top = x2.shape[0], tuple(x.shape[:-1]), weight.shape[0], int(n_top)
    w = _contig(weight.detach().to(x2.dtype), x2.dtype, "weight")
    if u is not None:
        u = _contig(u.detach().reshape(-1), torch.float32, "u")
        if u.numel() != n:
            raise ValueError(f"next_token: {u.numel()} uniform numbers for {n} rows")
    elif not greedy:
        u = torch.rand(n, dtype=torch.float32, device=dev)
    token = torch.empty(n, dtype=torch.int64, device=dev)
    prob = torch.empty(n, dtype=torch.float32, device=dev)
    kept = torch.empty(n, dtype=torch.int32, device=dev)
    top_cls = torch.empty((n, n_top), dtype=torch.int32, device=dev) if n_top > 0 else None
    top_prob = torch.empty((n, n_top), dtype=torch.float32, device=dev) if n_top > 0 else None
    logits = torch.empty((n, vocab), dtype=torch.float32, device=dev) if return_logits else None
    d = capi.MotNextTokenDesc()
    d.struct_size = C.sizeof(capi.MotNextTokenDesc)
    d.dtype, d.norm_in, d.greedy, d.n_rows, d.x_stride = capi.dtype_code(x2.dtype), int(bool(norm_in)), int(bool(greedy)), n, stride
    d.model_dim, d.vocab, d.eps, d.temperature = x2.shape[1], vocab, 0.0, float(temperature)
    d.top_k, d.top_p, d.n_top, d.reserved = int(top_k), float(top_p), n_top, 0
    d.x, d.weight, d.u, d.token, d.prob, d.kept = capi.ptr(x2), capi.ptr(w), capi.ptr(u), capi.ptr(token), capi.ptr(prob), capi.ptr(kept)
    d.top_cls, d.top_prob, d.logits = capi.ptr(top_cls), capi.ptr(top_prob), capi.ptr(logits)
    if n > 0:   # no rows: nothing to launch (and an empty tensor has no address to pass)
        _launch(dev, d, capi.lib.mot_next_token, ws_bytes=capi.lib.mot_next_token_workspace_bytes)
    return NextToken(token.reshape(shape), prob.reshape(shape), kept.reshape(shape),
                     None if top_cls is None else top_cls.reshape(shape + (n_top,)), None if top_prob is None else top_prob.reshape(shape + (n_top,)),
                     None if logits is None else logits.reshape(shape + (vocab,)))


def window_targets(targets: torch.Tensor, ranges, ignore_index: int = -100) -> torch.Tensor:
    """targets (B, T) with everything outside each row's [start, end) set to ignore_index: the positions slice_logits_and_targets
    (mathblations/data.py:262-278) keeps for y_indices = ranges, (B, 2) as a tensor or a sequence of (start, end).  The mean over the
    kept targets of plain_head_loss on the result is the reference's cross_entropy over the sliced rows.  Plain torch on the targets'
    device, no loop over rows."""
    if targets.ndim != 2:
        raise ValueError(f"window_targets: targets must be (B, T), got {tuple(targets.shape)}")
    r = torch.as_tensor(ranges, device=targets.device).reshape(targets.shape[0], 2)
    pos = torch.arange(targets.shape[1], device=targets.device)
    inside = (pos >= r[:, :1]) & (pos < r[:, 1:])
    return torch.where(inside, targets, torch.full_like(targets, ignore_index))


def window_kept_bound(ranges, seq_len: int) -> int:
    """The number of positions window_targets keeps for `ranges` on sequences of seq_len positions: the sum over the rows of
    clip(end, 0, seq_len) - clip(start, 0, seq_len), a negative length counting 0.  The max_kept of plain_head_loss /
    plain_head_eval for targets marked with window_targets (when every target inside the windows is a class; fewer kept rows only
    leave padding).  ranges: a sequence of (start, end) pairs or a CPU tensor (B, 2): host data, read on the host.  A tensor on
    another device raises TypeError: there is no hidden device read here; take the bound from the loader's host copy."""
    if isinstance(ranges, torch.Tensor) and ranges.device.type != "cpu":
        raise TypeError(f"window_kept_bound: ranges must be host data (a sequence or a CPU tensor), got a tensor on {ranges.device}")
    r = torch.as_tensor(ranges, dtype=torch.int64).reshape(-1, 2).clamp(0, int(seq_len))
    return int((r[:, 1] - r[:, 0]).clamp_min(0).sum())


# ----------------------------------------------------------------------------------------------
# byte self-attention in front of the concat mixin: ByteSelfAttn with use_byte_self_attn, train_gpt.py:382-418
# ----------------------------------------------------------------------------------------------
def _byte_self_attn_desc(x3, qkv_w, proj_w, lam, cos, sin, bpt, window, block_causal, out, saved):
    dev = capi.require_device(x3, qkv_w, proj_w, lam, cos, sin)
    B, L, D = x3.shape
    d = capi.MotByteSelfAttnDesc()
    d.struct_size = C.sizeof(capi.MotByteSelfAttnDesc)
    d.dtype, d.n_rows, d.row_len, d.bpt, d.window, d.block_causal = capi.F32, B, L, int(bpt), int(window), int(bool(block_causal))
    d.dim, d.n_heads, d.head_dim = D, qkv_w.shape[1] // 128, 128
    d.x, d.qkv_w, d.proj_w, d.lambda_v = capi.ptr(x3), capi.ptr(qkv_w), capi.ptr(proj_w), capi.ptr(lam)
    d.cos, d.sin, d.rope_rows, d.eps = capi.ptr(cos), capi.ptr(sin), cos.shape[0], 0.0
    d.out = capi.ptr(out)
    if saved is not None:
        d.saved, d.saved_bytes = capi.ptr(saved), saved.numel()
    return d, dev


class _ByteSelfAttnFn(torch.autograd.Function):
    """forward = mot_byte_self_attn_fwd (out, and the saved projections / attention output / row statistics),
    backward = mot_byte_self_attn_bwd (dx, d qkv_w, d c_proj.weight, d lambdas[0])."""

    @staticmethod
    def forward(ctx, x, qkv_w, proj_w, lambdas, cos, sin, bpt, window, block_causal):
        for t, what in ((x, "x"), (qkv_w, "qkv_w"), (proj_w, "proj_w"), (lambdas, "lambdas")):
            if t.is_cuda and t.dtype != torch.float32:
                raise NotImplementedError(f"byte_self_attn: {what} is {t.dtype}; only float32 is built (bfloat16 byte embeddings, the "
                                          "production cast of train_gpt.py:1124-1126, are the follow-up)")
        capi.require_device(x, qkv_w, proj_w, lambdas, cos, sin)
        if x.ndim != 3 or qkv_w.ndim != 3 or qkv_w.shape[0] != 3 or qkv_w.shape[2] != x.shape[2] or qkv_w.shape[1] % 128:
            raise ValueError(f"byte_self_attn: x (B, L, D) and qkv_w (3, heads * 128, D) expected, got {tuple(x.shape)} and {tuple(qkv_w.shape)}")
        if tuple(proj_w.shape) != (x.shape[2], qkv_w.shape[1]) or lambdas.numel() != 2:
            raise ValueError("byte_self_attn: proj_w must be (D, heads * 128) and lambdas a 2-vector")
        x3 = _contig(x.detach(), torch.float32, "x")
        w, pw = _contig(qkv_w.detach(), torch.float32, "qkv_w"), _contig(proj_w.detach(), torch.float32, "proj_w")
        lam = _contig(lambdas.detach(), torch.float32, "lambdas")
        cs, sn = _contig(cos, torch.float32, "cos"), _contig(sin, torch.float32, "sin")
        out = torch.empty_like(x3)
        d, dev = _byte_self_attn_desc(x3, w, pw, lam, cs, sn, bpt, window, block_causal, out, None)
        saved = torch.empty(int(capi.lib.mot_byte_self_attn_saved_bytes(C.byref(d))), dtype=torch.uint8, device=dev)
        d.saved, d.saved_bytes = capi.ptr(saved), saved.numel()
        _launch(dev, d, capi.lib.mot_byte_self_attn_fwd)
        ctx.save_for_backward(x3, w, pw, lam, cs, sn, saved)
        ctx.cfg = (bpt, window, block_causal)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x3, w, pw, lam, cs, sn, saved = ctx.saved_tensors
        bpt, window, block_causal = ctx.cfg
        d, dev = _byte_self_attn_desc(x3, w, pw, lam, cs, sn, bpt, window, block_causal, None, saved)
        go = _contig(grad_out.detach(), torch.float32, "grad_out")
        need = ctx.needs_input_grad
        dx = torch.empty_like(x3) if need[0] else None
        dw = torch.empty_like(w) if need[1] else None
        dpw = torch.empty_like(pw) if need[2] else None
        dlam = torch.zeros(2, dtype=torch.float32, device=dev) if need[3] else None   # lambdas[1] takes no part: its gradient is 0
        g = capi.MotByteSelfAttnGrads()
        g.struct_size = C.sizeof(capi.MotByteSelfAttnGrads)
        g.grad_out, g.dx, g.d_qkv_w, g.d_proj_w, g.d_lambda = capi.ptr(go), capi.ptr(dx), capi.ptr(dw), capi.ptr(dpw), capi.ptr(dlam)
        _launch(dev, d, capi.lib.mot_byte_self_attn_bwd, C.byref(g), ws_bytes=capi.lib.mot_byte_self_attn_workspace_bytes)
        return dx, dw, dpw, dlam, None, None, None, None, None


@torch.compiler.disable
def byte_self_attn(x: torch.Tensor, qkv_w: torch.Tensor, proj_w: torch.Tensor, lambdas: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, *,
                   bpt: int, window: int, block_causal: bool = False) -> torch.Tensor:
    """ByteSelfAttn.forward with use_byte_self_attn (train_gpt.py:382-418): x + CausalSelfAttention(x, None, block_mask) for x (B, L, D),
    L = T * bpt byte positions per batch row.  qkv_w (3, heads * 128, D), proj_w = c_proj.weight (D, heads * 128), lambdas the module's
    2-vector (the first entry scales v; the second takes no part and gets a zero gradient), cos / sin the Rotary buffers (>= L, 64).
    `window` is in bytes (sliding_window_tokens * bpt, at most 256); block_causal = mix_byte_in_tok.  float32; differentiable in x,
    qkv_w, proj_w and lambdas.  A non-contiguous x is copied."""
    return _ByteSelfAttnFn.apply(x, qkv_w, proj_w, lambdas, cos, sin, int(bpt), int(window), bool(block_causal))


# ------------------------------------------------------------------------------------------------
# linear-on-bytes mixin (modded-nanogpt/runs/71051_*.py:225-229): x = norm(E_tok[tok] + byte_fc . cat_k E_byte[id_k])
# ------------------------------------------------------------------------------------------------
_BYTE_FC_COMPOSED = bool(os.environ.get("MOT_BYTE_FC_COMPOSED"))   # kernel-selection switch, read once at import like _ENV_FLAGS above


def _byte_fc_desc(tokens, tok_table, byte_table, byte_fc, bpt, norm_out, eps):
    """The descriptor's problem part, checked: tokens (B, T) int32 contiguous, the three float tensors of one dtype."""
    tok = _tokens_2d(tokens)
    tt = _table(tok_table, "tok_table")
    bt = _table(byte_table, "byte_table", tt.dtype)
    w = _table(byte_fc, "byte_fc", tt.dtype)
    if tt.ndim != 2 or bt.ndim != 2 or w.ndim != 2 or tuple(w.shape) != (tt.shape[1], int(bpt) * bt.shape[1]):
        raise ValueError(f"byte_fc must be (model_dim, bpt*byte_dim) = ({tt.shape[1]}, {int(bpt)}*{bt.shape[1]}), got {tuple(w.shape)}")
    B, T = tok.shape
    d = capi.MotByteFcMixDesc()
    d.struct_size = C.sizeof(capi.MotByteFcMixDesc)
    d.dtype = capi.dtype_code(tt.dtype)
    d.n_rows, d.tokens_per_row, d.bpt = B, T, int(bpt)
    d.tokens = capi.ptr(tok)
    d.tok_table, d.tok_rows, d.tok_dim, d.model_dim = capi.ptr(tt), tt.shape[0], tt.shape[1], tt.shape[1]
    d.byte_table, d.byte_rows, d.byte_dim = capi.ptr(bt), bt.shape[0], bt.shape[1]
    d.byte_fc = capi.ptr(w)
    d.norm_out, d.eps = int(bool(norm_out)), float(eps or 0.0)
    return d, tok, [tok, tt, bt, w]


@torch.compiler.disable
def _byte_fc_mix_fwd(tokens, tok_table, byte_table, byte_fc, *, bpt, ids=None, ttb=None, pull=None, pad_byte=456, eot_byte=457,
                     norm_out=True, eps=None, return_ids=False, counters=None, row_rnorm=None, composed=None):
    dev = capi.require_device(tokens, tok_table, byte_table, byte_fc, ids, ttb)
    d, tok, keep = _byte_fc_desc(tokens, tok_table, byte_table, byte_fc, bpt, norm_out, eps)
    d.flags = capi.BYTE_FC_COMPOSED if (_BYTE_FC_COMPOSED if composed is None else composed) else 0
    B, T = tok.shape
    ids_padded = ids_pulled = None
    _bind_byte_ids(d, keep, B=B, T=T, bpt=bpt, ids=ids, ttb=ttb, pull=pull, what="byte_fc_mix")
    if ttb is not None and return_ids:
        ids_padded, ids_pulled = _new_ids(B, T, bpt, dev), _new_ids(B, T, bpt, dev)
        d.out_ids_padded, d.out_ids_pulled = capi.ptr(ids_padded), capi.ptr(ids_pulled)
    d.pad_byte, d.eot_byte = int(pad_byte), int(eot_byte)
    out = torch.empty((B, T, d.model_dim), dtype=tok_table.dtype, device=dev)
    if B * T == 0:   # an empty batch: nothing to launch (torch hands out null pointers for empty tensors, which the C validation refuses)
        return MixResult(out, ids_padded, ids_pulled) if return_ids else out
    d.out = capi.ptr(out)
    _bind_counters(d, counters, dev)
    if row_rnorm is not None:
        assert row_rnorm.dtype == torch.float32 and row_rnorm.numel() == B * T and row_rnorm.is_contiguous()
        d.out_row_rnorm = capi.ptr(row_rnorm)
    _launch(dev, d, capi.lib.mot_byte_fc_mix_fwd, ws_bytes=capi.lib.mot_byte_fc_mix_workspace_bytes)
    return MixResult(out, ids_padded, ids_pulled) if return_ids else out


@torch.compiler.disable
def byte_fc_mix_backward(grad_out, tokens, tok_table, byte_table, byte_fc, *, bpt, ids, norm_out=True, eps=None, out=None, row_rnorm=None,
                         token_order=None, into=None) -> dict:
    """One call of mot_byte_fc_mix_bwd.  Returns dense fp32 gradients {tok_table, byte_table, byte_fc} -- fp32 also for bfloat16
    parameters (the autograd node rounds once); `into` (same keys, fp32) accumulates into existing buffers.  With norm_out the
    float32 backward needs the forward's output `out` and its `row_rnorm`; the bfloat16 backward forms the pre-norm row again
    and reads neither (include/mot.h).  `token_order` as in :func:`embed_mix_backward`."""
    dev = capi.require_device(grad_out, tokens, tok_table, byte_table, byte_fc, ids, out, row_rnorm)
    d, tok, keep = _byte_fc_desc(tokens, tok_table, byte_table, byte_fc, bpt, norm_out, eps)
    B, T = tok.shape
    dt = tok_table.dtype
    g = _contig(grad_out, dt, "grad_out")
    ia = _contig(ids, torch.int64, "ids")
    if g.numel() != B * T * d.model_dim or ia.numel() != B * T * bpt:
        raise ValueError("grad_out must be (B, T, model_dim) and ids (B, T*bpt)")
    keep += [g, ia]
    d.id_source, d.ids = capi.IDS_GIVEN, capi.ptr(ia)
    if norm_out and dt == torch.float32:
        if out is None or row_rnorm is None:
            raise ValueError("byte_fc_mix backward with norm_out needs the forward's output and row_rnorm")
        xo = _contig(out, dt, "out")
        keep.append(xo)
        d.out, d.out_row_rnorm = capi.ptr(xo), capi.ptr(row_rnorm)
    into = into or {}
    res = {}
    for k, p in (("tok_table", tok_table), ("byte_table", byte_table), ("byte_fc", byte_fc)):
        res[k] = into[k] if into.get(k) is not None else torch.zeros(p.shape, dtype=torch.float32, device=dev)
    if B * T == 0:   # an empty batch adds nothing
        return res
    gr = capi.MotByteFcMixGrads()
    gr.struct_size = C.sizeof(capi.MotByteFcMixGrads)
    gr.grad_out, gr.d_tok, gr.d_byte, gr.d_byte_fc = capi.ptr(g), capi.ptr(res["tok_table"]), capi.ptr(res["byte_table"]), capi.ptr(res["byte_fc"])
    _bind_token_order(gr, keep, token_order, B * T, tok_table.shape[0], dev)
    _launch(dev, d, capi.lib.mot_byte_fc_mix_bwd, C.byref(gr), ws_bytes=capi.lib.mot_byte_fc_mix_bwd_workspace_bytes)
    return res


class _ByteFcMixFn(torch.autograd.Function):
    """Autograd node of the linear-on-bytes mixin: one mot_byte_fc_mix_fwd call forward, one mot_byte_fc_mix_bwd call backward for
    the two tables and byte_fc.  Saved: the byte ids and, for float32 tensors, the output and the per-row factor (4 bytes per token);
    u is gathered again."""

    @staticmethod
    def forward(ctx, tok_table, byte_table, byte_fc, tokens, kw):
        kw = dict(kw)
        user_return_ids = kw.pop("return_ids", False)
        from_ttb = kw.get("ttb") is not None
        t2 = tokens if tokens.ndim == 2 else tokens[None]
        saves_x = kw.get("norm_out", True) and tok_table.dtype == torch.float32
        rn = torch.empty(t2.shape, dtype=torch.float32, device=tok_table.device) if saves_x else None
        r = _byte_fc_mix_fwd(tokens, tok_table.detach(), byte_table.detach(), byte_fc.detach(), return_ids=from_ttb or user_return_ids,
                             row_rnorm=rn, **kw)
        x = r.x if isinstance(r, MixResult) else r
        ids = kw.get("ids")
        if from_ttb:
            ids = r.ids_pulled if kw.get("pull") not in (None, "none") else r.ids_padded
        ctx.order = _token_orders.get(tokens, tok_table.shape[0]) if _HOIST_SORT else None
        ctx.save_for_backward(tok_table, byte_table, byte_fc, tokens, ids, x if rn is not None else None, rn)
        ctx.kw = dict(bpt=kw["bpt"], norm_out=kw.get("norm_out", True), eps=kw.get("eps"))
        if user_return_ids:
            ctx.mark_non_differentiable(r.ids_padded, r.ids_pulled)
            return x, r.ids_padded, r.ids_pulled
        return x

    @staticmethod
    def backward(ctx, gx, *_):
        tok_table, byte_table, byte_fc, tokens, ids, x, rn = ctx.saved_tensors
        g = byte_fc_mix_backward(gx, tokens, tok_table.detach(), byte_table.detach(), byte_fc.detach(), ids=ids,
                                 out=None if x is None else x.detach(), row_rnorm=rn, token_order=_ready_order(ctx.order, gx.device), **ctx.kw)
        return _grad_like(g["tok_table"], tok_table), _grad_like(g["byte_table"], byte_table), _grad_like(g["byte_fc"], byte_fc), None, None


def byte_fc_mix(tokens: torch.Tensor, tok_table: torch.Tensor, byte_table: torch.Tensor, byte_fc: torch.Tensor, *, bpt: int,
                ids: torch.Tensor | None = None, ttb: torch.Tensor | None = None, pull: str | None = None, pad_byte: int = 456,
                eot_byte: int = 457, norm_out: bool = True, eps: float | None = None, return_ids: bool = False, composed: bool | None = None):
    """The linear-on-bytes mixin of modded-nanogpt/runs/71051_*.py:225-229: ``x = norm(tok_table[tokens] + cat_k byte_table[ids[:, k]] @
    byte_fc.T)`` with byte_fc (model_dim, bpt * byte_dim) in nn.Linear layout, no bias; float32 or bfloat16 throughout (bf16: fp32
    arithmetic, rounded where the reference's bf16 run rounds).  tokens (B, T) or (T,); the byte ids are given as `ids` (B, T*bpt)
    int64 or come from the token->byte table `ttb` (+ `pull` = "left" | "right" | None) inside the call.  `eps` None is the float32
    epsilon for both dtypes, which is what F.rms_norm(eps=None) applies to bfloat16 rows as well; pass ``2.0 ** -7`` for
    torch.finfo(bfloat16).eps.  One autograd node covers the two tables and byte_fc; `return_ids` returns a MixResult.  `composed`
    (bfloat16 forward: the separate gather / product / row-pass kernels instead of the one gather-GEMM) overrides the import-time
    default (MotByteFcMixDesc.flags)."""
    kw = dict(bpt=bpt, ids=ids, ttb=ttb, pull=pull, pad_byte=pad_byte, eot_byte=eot_byte, norm_out=norm_out, eps=eps, return_ids=return_ids,
              composed=composed)
    if not (tok_table.dtype == byte_table.dtype == byte_fc.dtype):
        raise TypeError(f"byte_fc_mix: tok_table {tok_table.dtype}, byte_table {byte_table.dtype} and byte_fc {byte_fc.dtype} must share one dtype")
    capi.dtype_code(tok_table.dtype)
    capi.require_device(tokens, tok_table, byte_table, byte_fc, ids, ttb)
    if torch.is_grad_enabled() and any(p.requires_grad for p in (tok_table, byte_table, byte_fc)):
        r = _ByteFcMixFn.apply(tok_table, byte_table, byte_fc, tokens, kw)
        return MixResult(*r) if return_ids else r
    return _byte_fc_mix_fwd(tokens, tok_table, byte_table, byte_fc, **kw)


# ------------------------------------------------------------------------------------------------
# bytes-only front-end and byte value embeddings (modded-nanogpt/runs/5_bytes-in_bytes-valemb.py:225-232, 248, 305, 314):
# out_j = norm_j?(cat_k table_j[id_k]) for up to four tables over one id stream, no token row
# ------------------------------------------------------------------------------------------------
def _byte_cat_desc(tables, norm, bpt, eps, tokens, ids, what):
    """The descriptor's problem part, checked: 1..4 contiguous (rows, byte_dim) tables of one dtype, a bool per table, and the
    batch shape (B, T) from the tokens or, without them, from the ids."""
    tables = list(tables)
    norm = [bool(x) for x in norm]
    if not 1 <= len(tables) <= capi.BYTE_CAT_MAX_OUT:
        raise ValueError(f"{what}: {len(tables)} tables, 1..{capi.BYTE_CAT_MAX_OUT} are built")
    if len(norm) != len(tables):
        raise ValueError(f"{what}: norm needs one bool per table ({len(tables)}), got {len(norm)}")
    dt = tables[0].dtype
    tabs = [_table(t, f"{what}: table {j}") for j, t in enumerate(tables)]
    for j, t in enumerate(tabs):
        if t.dtype != dt:
            raise TypeError(f"{what}: table {j} is {t.dtype} but table 0 is {dt}: all tables share one dtype")
        if t.ndim != 2 or t.shape[1] != tabs[0].shape[1]:
            raise ValueError(f"{what}: table {j} must be (rows, byte_dim = {tabs[0].shape[1]}), got {tuple(t.shape)}")
    bpt = int(bpt)
    keep = list(tabs)
    tok = None
    if tokens is not None:
        tok = _tokens_2d(tokens)
        B, T = tok.shape
        keep.append(tok)
    else:
        if ids is None:
            raise ValueError(f"{what}: pass tokens (with ttb) or ids")
        i2 = ids[None] if ids.ndim == 1 else ids.reshape(ids.shape[0], -1)
        if i2.shape[1] % bpt:
            raise AssertionError(f"{what}: {i2.shape[1]} byte ids per row are not a multiple of bpt {bpt}")
        B, T = i2.shape[0], i2.shape[1] // bpt
    d = capi.MotByteCatDesc()
    d.struct_size = C.sizeof(capi.MotByteCatDesc)
    d.dtype = capi.dtype_code(dt)
    d.n_rows, d.tokens_per_row, d.bpt, d.byte_dim, d.n_out = B, T, bpt, tabs[0].shape[1], len(tabs)
    d.tokens = capi.ptr(tok)
    d.eps = float(eps or 0.0)
    for j, t in enumerate(tabs):
        d.slot[j].table, d.slot[j].rows, d.slot[j].norm, d.slot[j].dtype = capi.ptr(t), t.shape[0], int(norm[j]), d.dtype
    return d, tabs, keep, (B, T)


@torch.compiler.disable
def _byte_cat_fwd(tables, *, bpt, norm, tokens=None, ids=None, ttb=None, pull=None, pad_byte=456, eot_byte=457, eps=None, return_ids=False,
                  counters=None):
    dev = capi.require_device(*tables, tokens, ids, ttb)
    d, tabs, keep, (B, T) = _byte_cat_desc(tables, norm, bpt, eps, tokens, None if ttb is not None else ids, "byte_cat")
    ids_padded = ids_pulled = None
    if ttb is not None and tokens is None:
        raise ValueError("byte_cat: ids from the token->byte table need the tokens")
    _bind_byte_ids(d, keep, B=B, T=T, bpt=bpt, ids=ids, ttb=ttb, pull=pull, what="byte_cat")
    if ttb is not None:
        used_only = return_ids == "used"   # the autograd node: only the tensor the gathers index (8 * bpt bytes per token, written once)
        if return_ids and not (used_only and d.pull_dir != capi.PULL_NONE):
            ids_padded = _new_ids(B, T, bpt, dev)
            d.out_ids_padded = capi.ptr(ids_padded)
        if return_ids and not (used_only and d.pull_dir == capi.PULL_NONE):
            ids_pulled = _new_ids(B, T, bpt, dev)
            d.out_ids_pulled = capi.ptr(ids_pulled)
    d.pad_byte, d.eot_byte = int(pad_byte), int(eot_byte)
    outs = tuple(torch.empty((B, T, bpt * d.byte_dim), dtype=tabs[0].dtype, device=dev) for _ in tabs)
    if B * T == 0:   # an empty batch: nothing to launch
        return outs, ids_padded, ids_pulled
    for j, o in enumerate(outs):
        d.slot[j].out = capi.ptr(o)
    _bind_counters(d, counters, dev)
    _launch(dev, d, capi.lib.mot_byte_cat_fwd)
    return outs, ids_padded, ids_pulled


@torch.compiler.disable
def byte_cat_backward(grad_outs, tables, *, bpt, norm, ids, eps=None, into=None, counters=None) -> list:
    """One call of mot_byte_cat_bwd.  `grad_outs` holds one upstream gradient (B, T, bpt*byte_dim) or None per table; a table
    whose entry is None is skipped and gets None back.  Returns the dense fp32 table gradients -- fp32 also for bfloat16 tables
    (the autograd node rounds once); `into` (a list, fp32 tensors or None) accumulates into existing buffers.  Nothing of the
    forward is needed but the ids it used.  `counters` (int64[2] on the device, a measurement aid) is incremented by the number of
    non-zero gradient terms and by how many of them took the exact global path instead of the LDS sums."""
    grad_outs = list(grad_outs)
    dev = capi.require_device(*tables, ids, *[g for g in grad_outs if g is not None])
    d, tabs, keep, (B, T) = _byte_cat_desc(tables, norm, bpt, eps, None, ids, "byte_cat_backward")
    if len(grad_outs) != len(tabs):
        raise ValueError(f"byte_cat_backward: {len(grad_outs)} gradients for {len(tabs)} tables")
    ia = _contig(ids, torch.int64, "ids")
    keep.append(ia)
    d.id_source, d.ids = capi.IDS_GIVEN, capi.ptr(ia)
    gr = capi.MotByteCatGrads()
    gr.struct_size = C.sizeof(capi.MotByteCatGrads)
    into = list(into) if into is not None else [None] * len(tabs)
    res = []
    for j, (g, t) in enumerate(zip(grad_outs, tabs)):
        if g is None:
            res.append(None)
            continue
        gc = _contig(g, t.dtype, f"grad_outs[{j}]")
        if gc.numel() != B * T * bpt * d.byte_dim:
            raise ValueError(f"grad_outs[{j}] must be (B, T, bpt*byte_dim)")
        keep.append(gc)
        acc = into[j] if into[j] is not None else torch.zeros(t.shape, dtype=torch.float32, device=dev)
        if acc.dtype != torch.float32 or acc.shape != t.shape or not acc.is_contiguous():
            raise ValueError(f"into[{j}] must be a contiguous float32 tensor of the table's shape")
        res.append(acc)
        gr.slot[j].grad_out, gr.slot[j].d_table = capi.ptr(gc), capi.ptr(acc)
    if B * T == 0 or all(g is None for g in grad_outs):   # an empty batch adds nothing
        return res
    if counters is not None:
        if counters.dtype != torch.int64 or counters.numel() < 2 or counters.device != dev:
            raise ValueError("counters must be an int64[2] tensor on the inputs' device")
        d.counters = capi.ptr(counters)
    _launch(dev, d, capi.lib.mot_byte_cat_bwd, C.byref(gr), ws_bytes=capi.lib.mot_byte_cat_bwd_workspace_bytes)
    return res


class _ByteCatFn(torch.autograd.Function):
    """Autograd node of byte_cat: one mot_byte_cat_fwd call forward, one mot_byte_cat_bwd call backward for all tables.  Saved: the
    tables and the int64 byte ids (given, or written once by the forward); every row is gathered again."""

    @staticmethod
    def forward(ctx, kw, *tables):
        kw = dict(kw)
        user_return_ids = kw.pop("return_ids", False)
        from_ttb = kw.get("ttb") is not None
        outs, ids_padded, ids_pulled = _byte_cat_fwd([t.detach() for t in tables], return_ids=True if user_return_ids else ("used" if from_ttb else False),
                                                     **kw)
        ids = kw.get("ids")
        if from_ttb:
            ids = ids_pulled if kw.get("pull") not in (None, "none") else ids_padded
        ctx.save_for_backward(ids, *tables)
        ctx.set_materialize_grads(False)   # an output nothing depends on arrives as None and its table is skipped
        ctx.kw = dict(bpt=kw["bpt"], norm=tuple(kw["norm"]), eps=kw.get("eps"))
        ctx.n_out = len(tables)
        if user_return_ids and from_ttb:
            ctx.mark_non_differentiable(ids_padded, ids_pulled)
            return (*outs, ids_padded, ids_pulled)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        ids, *tables = ctx.saved_tensors
        gs = [g if ctx.needs_input_grad[1 + j] else None for j, g in enumerate(grads[:ctx.n_out])]
        if all(g is None for g in gs):
            return (None,) * (1 + ctx.n_out)
        res = byte_cat_backward(gs, [t.detach() for t in tables], ids=ids, **ctx.kw)
        # bf16 parameters get their gradient rounded once, from the fp32 sums
        return (None, *[_grad_like(r, t) for r, t in zip(res, tables)])


def byte_cat(tables, *, bpt: int, norm, tokens: torch.Tensor | None = None, ids: torch.Tensor | None = None, ttb: torch.Tensor | None = None,
             pull: str | None = None, pad_byte: int = 456, eot_byte: int = 457, eps: float | None = None, return_ids: bool = False):
    """The bytes-only front-end and the byte value embeddings of modded-nanogpt/runs/5_bytes-in_bytes-valemb.py:225-232, 248, 305,
    314: for each of the 1..4 `tables` (rows_j, byte_dim), all of one dtype (float32 or bfloat16), ``out_j = table_j[ids].reshape(B,
    T, bpt * byte_dim)``, rms-normalised over the last dimension where ``norm[j]`` is set (fp32 arithmetic, one rounding at the
    store; without the norm a bit-exact copy).  One launch serves every table.  The byte ids are given as `ids` (B, T*bpt) int64,
    or come from `tokens` (B, T) and the token->byte table `ttb` (+ `pull` = "left" | "right" | None) inside the call.  `eps` None
    is the float32 epsilon for both dtypes, which is what F.rms_norm(eps=None) applies to bfloat16 rows as well.  Returns a tuple
    of len(tables) tensors (B, T, bpt*byte_dim); with `return_ids` (ids from the table) the tuple, ids_padded and ids_pulled.  One
    autograd node covers all tables."""
    tables = list(tables)
    norm = tuple(bool(x) for x in norm)
    kw = dict(bpt=int(bpt), norm=norm, tokens=tokens, ids=ids, ttb=ttb, pull=pull, pad_byte=pad_byte, eot_byte=eot_byte, eps=eps,
              return_ids=return_ids)
    for j, t in enumerate(tables):
        if t.dtype != tables[0].dtype:
            raise TypeError(f"byte_cat: table {j} is {t.dtype} but table 0 is {tables[0].dtype}: all tables share one dtype")
    if tables:
        capi.dtype_code(tables[0].dtype)
    capi.require_device(*tables, tokens, ids, ttb)
    n = len(tables)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tables):
        r = _ByteCatFn.apply(kw, *tables)
        return (tuple(r[:n]), r[n], r[n + 1]) if return_ids and ttb is not None else tuple(r[:n])
    outs, ids_padded, ids_pulled = _byte_cat_fwd(tables, **kw)
    return (outs, ids_padded, ids_pulled) if return_ids and ttb is not None else outs


# ------------------------------------------------------------------------------------------------
# token value embeddings (scaled-pre-train/train_gpt.py:566, 600; modded-nanogpt/runs/71_*_toks-valemb.py:247, 303):
# out_j = table_j[tokens] for up to four tables of one shape over one token stream
# ------------------------------------------------------------------------------------------------
def _value_embeds_tokens(tokens, what):
    if tokens.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{what}: tokens must be int32 or int64, got {tokens.dtype}")
    if tokens.ndim not in (1, 2):
        raise ValueError(f"{what}: tokens must be (T,) or (B, T), got {tuple(tokens.shape)}")
    return _int32(tokens)


def _value_embeds_desc(tok, n_tables, rows, dim, dtype, what):
    if not 1 <= n_tables <= capi.VALUE_EMBEDS_MAX_TABLES:
        raise ValueError(f"{what}: {n_tables} tables, 1..{capi.VALUE_EMBEDS_MAX_TABLES} are built")
    d = capi.MotValueEmbedsDesc()
    d.struct_size = C.sizeof(capi.MotValueEmbedsDesc)
    d.dtype = capi.dtype_code(dtype)
    d.n_tokens, d.tokens, d.tok_rows, d.dim, d.n_tables = tok.numel(), capi.ptr(tok), int(rows), int(dim), n_tables
    return d


def _value_embeds_tables(tables, what):
    """1..4 (rows, dim) tables of one shape and dtype; a contiguous table is used where it lives (no copy)."""
    tables = list(tables)
    if not tables:
        raise ValueError(f"{what}: no tables")
    dt = tables[0].dtype
    for j, t in enumerate(tables):
        if t.dtype != dt:
            raise TypeError(f"{what}: table {j} is {t.dtype} but table 0 is {dt}: all tables share one dtype")
        if t.ndim != 2 or t.shape != tables[0].shape:
            raise ValueError(f"{what}: table {j} must be (rows, dim) = {tuple(tables[0].shape)}, got {tuple(t.shape)}")
    return [_table(t, f"{what}: table {j}") for j, t in enumerate(tables)]


@torch.compiler.disable
def _value_embeds_fwd(tokens, tables):
    dev = capi.require_device(tokens, *tables)
    tabs = _value_embeds_tables(tables, "value_embeds")
    tok = _value_embeds_tokens(tokens, "value_embeds")
    rows, dim = tabs[0].shape
    d = _value_embeds_desc(tok, len(tabs), rows, dim, tabs[0].dtype, "value_embeds")
    outs = tuple(torch.empty(tuple(tokens.shape) + (dim,), dtype=tabs[0].dtype, device=dev) for _ in tabs)
    if tok.numel() == 0:   # an empty batch: nothing to launch
        return outs
    for j, (t, o) in enumerate(zip(tabs, outs)):
        d.tables[j], d.outs[j] = capi.ptr(t), capi.ptr(o)
    _launch(dev, d, capi.lib.mot_value_embeds_fwd)
    return outs


@torch.compiler.disable
def _value_embeds_bwd(grad_outs, tokens, rows, dim, dtype, token_order, out=None):
    grad_outs = list(grad_outs)
    out = list(out) if out is not None else [None] * len(grad_outs)
    if len(out) != len(grad_outs):
        raise ValueError(f"value_embeds_backward: {len(out)} buffers in `out` for {len(grad_outs)} tables")
    dev = capi.require_device(tokens, token_order, *[g for g in grad_outs if g is not None])
    tok = _value_embeds_tokens(tokens, "value_embeds_backward")
    d = _value_embeds_desc(tok, len(grad_outs), rows, dim, dtype, "value_embeds_backward")
    gr = capi.MotValueEmbedsGrads()
    gr.struct_size = C.sizeof(capi.MotValueEmbedsGrads)
    keep, res = [tok], []
    n = tok.numel()
    for j, g in enumerate(grad_outs):
        if g is None:
            res.append(None)
            continue
        gc = _contig(g, dtype, f"grad_outs[{j}]")
        if gc.numel() != n * dim:
            raise ValueError(f"grad_outs[{j}] must be tokens.shape + ({dim},), got {tuple(g.shape)}")
        keep.append(gc)
        # written once by the call, every element: nothing to zero (an empty batch launches nothing and is all zeros)
        dt = out[j]
        if dt is None:
            dt = (torch.empty if n else torch.zeros)((rows, dim), dtype=dtype, device=dev)
        elif dt.dtype != dtype or tuple(dt.shape) != (rows, dim) or not dt.is_contiguous() or dt.device != dev:
            raise ValueError(f"out[{j}] must be a contiguous {dtype} tensor of the table's shape ({rows}, {dim}) on {dev}")
        elif n == 0:
            dt.zero_()
        res.append(dt)
        gr.grad_outs[j], gr.d_tables[j] = capi.ptr(gc), capi.ptr(dt)
    if n == 0 or all(g is None for g in grad_outs):
        return res
    _bind_token_order(gr, keep, token_order, n, rows, dev, contiguous="")
    _launch(dev, d, capi.lib.mot_value_embeds_bwd, C.byref(gr), ws_bytes=capi.lib.mot_value_embeds_bwd_workspace_bytes)
    return res


@torch.compiler.disable
def value_embeds_backward(grad_outs, tokens: torch.Tensor, tables, *, token_order: torch.Tensor | None = None, out=None) -> list:
    """One call of mot_value_embeds_bwd.  `grad_outs` holds one upstream gradient ``tokens.shape + (dim,)`` or None per table; a
    table whose entry is None is skipped and gets None back.  Returns the dense table gradients in the TABLES' dtype: each is the
    fp32 sum of its positions' rows rounded once, rows of absent ids are +0, and every element is written exactly once by the call
    (nothing is zeroed first, nothing accumulated).  The same inputs give the same bits on every run, with or without
    `token_order` (what :func:`token_order` returned for these tokens and this table height; the caller orders streams).  `out` (a
    list: a tensor of the table's shape and dtype, or None, per table) names buffers to write the gradients INTO instead of fresh
    ones -- overwritten, not accumulated, whatever they held; the buffer of a table whose gradient is None is not touched."""
    tabs = _value_embeds_tables(tables, "value_embeds_backward")
    grad_outs = list(grad_outs)
    if len(grad_outs) != len(tabs):
        raise ValueError(f"value_embeds_backward: {len(grad_outs)} gradients for {len(tabs)} tables")
    capi.require_device(tokens, *tabs)
    return _value_embeds_bwd(grad_outs, tokens, tabs[0].shape[0], tabs[0].shape[1], tabs[0].dtype, token_order, out)


class _ValueEmbedsFn(torch.autograd.Function):
    """Autograd node of value_embeds: one mot_value_embeds_fwd call forward, one mot_value_embeds_bwd call backward for all
    tables.  Saved: the tokens only (the gradient does not read the tables); the token order comes from the cache the fused
    front-end uses, so a step that feeds one token tensor to both sorts it once."""

    @staticmethod
    def forward(ctx, tokens, *tables):
        outs = _value_embeds_fwd(tokens, [t.detach() for t in tables])
        ctx.order = _token_orders.get(tokens, tables[0].shape[0]) if _HOIST_SORT and tokens.numel() else None
        ctx.save_for_backward(tokens)
        ctx.set_materialize_grads(False)   # an output nothing depends on arrives as None and its table is skipped
        ctx.meta = (tables[0].shape[0], tables[0].shape[1], tables[0].dtype, len(tables))
        return outs

    @staticmethod
    def backward(ctx, *grads):
        tokens, = ctx.saved_tensors
        rows, dim, dtype, n = ctx.meta
        gs = [g if ctx.needs_input_grad[1 + j] else None for j, g in enumerate(grads[:n])]
        if all(g is None for g in gs):
            return (None,) * (1 + n)
        return (None, *_value_embeds_bwd(gs, tokens, rows, dim, dtype, _ready_order(ctx.order, tokens.device)))


def value_embeds(tokens: torch.Tensor, tables) -> tuple:
    """The token value embeddings of scaled-pre-train/train_gpt.py:566 / 600 and modded-nanogpt/runs/71_*_toks-valemb.py:247 /
    303, ``[value_embed(tokens) for value_embed in value_embeds]``, in one launch: for each of the 1..4 `tables` (vocab, dim), all
    of one shape and dtype (float32 or bfloat16), ``out_j = table_j[tokens]``, a bit-exact copy.  `tokens` is (T,) or (B, T), int32
    or int64; each output has shape ``tokens.shape + (dim,)``.  One autograd node covers all tables; its backward writes each table
    gradient once, in the table's dtype, with the same bits on every run (see :func:`value_embeds_backward`)."""
    tables = list(tables)
    if isinstance(tokens, torch.Tensor) and all(isinstance(t, torch.Tensor) for t in tables):
        capi.require_device(tokens, *tables)
    _value_embeds_tables(tables, "value_embeds")
    if torch.is_grad_enabled() and any(t.requires_grad for t in tables):
        return tuple(_ValueEmbedsFn.apply(tokens, *tables))
    return _value_embeds_fwd(tokens, tables)


# ------------------------------------------------------------------------------------------------
# mixture-of-tokenizers value embeddings (modded-nanogpt/runs/9_mot-in_mot-valemb.py:225-235, 252-254, 310-313; runs 3 and 6):
# ve_j = norm(W_j . cat(Vt_j[tok], Vb_j[id_0], ..., Vb_j[id_{bpt-1}])) for up to four slots over one token and one id stream
# ------------------------------------------------------------------------------------------------
def _value_mix_desc(tokens, tok_tables, byte_tables, weights, bpt, norm_out, eps, what):
    """The descriptor's problem part, checked: tokens (B, T) int32 contiguous; per slot a (tok_rows, token_dim) table, a
    (byte_rows, byte_dim) table and an (out_dim, token_dim + bpt*byte_dim) weight, all of one dtype and of one shape per kind."""
    tt, bt, ws = list(tok_tables), list(byte_tables), list(weights)
    if not (len(tt) == len(bt) == len(ws)):
        raise ValueError(f"{what}: {len(tt)} token tables, {len(bt)} byte tables and {len(ws)} weights: one of each per slot")
    if not 1 <= len(tt) <= capi.VALUE_MIX_MAX_SLOTS:
        raise ValueError(f"{what}: {len(tt)} slots, 1..{capi.VALUE_MIX_MAX_SLOTS} are built")
    dt = tt[0].dtype
    for kind, ts in (("token table", tt), ("byte table", bt), ("weight", ws)):
        for j, t in enumerate(ts):
            if t.dtype != dt:
                raise TypeError(f"{what}: {kind} {j} is {t.dtype} but token table 0 is {dt}: all tensors share one dtype")
            if t.ndim != 2 or t.shape != ts[0].shape:
                raise ValueError(f"{what}: {kind} {j} must be 2-D of shape {tuple(ts[0].shape)}, got {tuple(t.shape)}")
    capi.dtype_code(dt)
    Dt, Db, Do = tt[0].shape[1], bt[0].shape[1], ws[0].shape[0]
    if ws[0].shape[1] != Dt + int(bpt) * Db:
        raise ValueError(f"{what}: weights must be (out_dim, token_dim + bpt*byte_dim) = (*, {Dt} + {int(bpt)}*{Db}), got {tuple(ws[0].shape)}")
    tok = _tokens_2d(tokens, f"{what}: tokens must be (B, T) or (T,)")
    tt, bt, ws = ([_table(t, f"{what}: {k} {j}") for j, t in enumerate(ts)] for k, ts in (("token table", tt), ("byte table", bt), ("weight", ws)))
    d = capi.MotValueMixDesc()
    d.struct_size = C.sizeof(capi.MotValueMixDesc)
    d.dtype = capi.dtype_code(dt)
    d.n_rows, d.tokens_per_row, d.bpt = tok.shape[0], tok.shape[1], int(bpt)
    d.tokens = capi.ptr(tok)
    d.tok_rows, d.byte_rows, d.token_dim, d.byte_dim, d.out_dim, d.n_slots = tt[0].shape[0], bt[0].shape[0], Dt, Db, Do, len(tt)
    d.norm_out, d.eps = int(bool(norm_out)), float(eps or 0.0)
    for j in range(len(tt)):
        d.slot[j].tok_table, d.slot[j].byte_table, d.slot[j].weight = capi.ptr(tt[j]), capi.ptr(bt[j]), capi.ptr(ws[j])
    return d, tok, [tok, tt, bt, ws]


_IDS_PER_TOKEN = "{}: byte ids must hold bytes_per_token ids per token, in per-token order (.., T*bpt)"   # value_mix and split_x0


@torch.compiler.disable
def _value_mix_fwd(tokens, tok_tables, byte_tables, weights, *, bpt, ids=None, ttb=None, pull=None, pad_byte=456, eot_byte=457, norm_out=True,
                   eps=None, save=False):
    """One mot_value_mix_fwd call.  Returns (outs, ids_used, row_rnorms): with `save` the ids the tables were read with (the given
    ones, or those made from `ttb`) and each slot's fp32 row factors, which the backward wants; (outs, None, None) otherwise."""
    dev = capi.require_device(tokens, *tok_tables, *byte_tables, *weights, ids, ttb)
    d, tok, keep = _value_mix_desc(tokens, tok_tables, byte_tables, weights, bpt, norm_out, eps, "value_mix")
    B, T = tok.shape
    outs = tuple(torch.empty(tuple(tokens.shape) + (d.out_dim,), dtype=tok_tables[0].dtype, device=dev) for _ in range(d.n_slots))
    ids_used = _bind_byte_ids(d, keep, B=B, T=T, bpt=bpt, ids=ids, ttb=ttb, pull=pull, what="value_mix", ids_what=_IDS_PER_TOKEN.format("value_mix"))
    if ttb is not None and save:
        ids_used = _new_ids(B, T, bpt, dev)
        d.out_ids = capi.ptr(ids_used)
    d.pad_byte, d.eot_byte = int(pad_byte), int(eot_byte)
    rns = None
    if save and norm_out:
        rns = tuple(torch.empty((B, T), dtype=torch.float32, device=dev) for _ in range(d.n_slots))
    if B * T == 0:   # an empty batch: nothing to launch
        return outs, ids_used, rns
    for j, o in enumerate(outs):
        d.slot[j].out = capi.ptr(o)
        if rns is not None:
            d.slot[j].out_row_rnorm = capi.ptr(rns[j])
    _launch(dev, d, capi.lib.mot_value_mix_fwd, ws_bytes=lambda p: capi.lib.mot_value_mix_workspace_bytes(p, 0))
    return outs, (ids_used if save else None), rns


@torch.compiler.disable
def value_mix_backward(grad_outs, tokens, tok_tables, byte_tables, weights, *, bpt, ids, norm_out=True, eps=None, outs=None, row_rnorms=None,
                       token_order=None) -> list:
    """One call of mot_value_mix_bwd.  `grad_outs` holds one upstream gradient ``tokens.shape + (out_dim,)`` or None per slot; a
    slot whose entry is None is skipped and gets None back.  Returns per slot a dict {tok_table, byte_table, weight}: the token
    table's gradient in the TABLES' dtype, every element written exactly once by the call (fp32 sums rounded once, +0 rows for
    absent ids, the same bits on every run, with or without `token_order`), the byte table's and the weight's as fresh fp32
    tensors (float atomics).  With norm_out the call reads the forward's outputs `outs` and their `row_rnorms`.  `ids` are the byte
    ids the forward used, `token_order` what :func:`token_order` returned for these tokens and the token tables' height."""
    grad_outs = list(grad_outs)
    dev = capi.require_device(tokens, *tok_tables, *byte_tables, *weights, ids, token_order, *[g for g in grad_outs if g is not None])
    d, tok, keep = _value_mix_desc(tokens, tok_tables, byte_tables, weights, bpt, norm_out, eps, "value_mix_backward")
    if len(grad_outs) != d.n_slots:
        raise ValueError(f"value_mix_backward: {len(grad_outs)} gradients for {d.n_slots} slots")
    _bind_byte_ids(d, keep, B=d.n_rows, T=d.tokens_per_row, bpt=bpt, ids=ids, ttb=None, pull=None, what="value_mix_backward",
                   ids_what=_IDS_PER_TOKEN.format("value_mix_backward"))
    n, dt = tok.numel(), tok_tables[0].dtype
    if norm_out and (outs is None or row_rnorms is None) and any(g is not None for g in grad_outs):
        raise ValueError("value_mix_backward with norm_out needs the forward's outputs and row_rnorms")
    gr = capi.MotValueMixGrads()
    gr.struct_size = C.sizeof(capi.MotValueMixGrads)
    res = []
    for j, g in enumerate(grad_outs):
        if g is None:
            res.append(None)
            continue
        gc = _contig(g, dt, f"grad_outs[{j}]")
        if gc.numel() != n * d.out_dim:
            raise ValueError(f"grad_outs[{j}] must be tokens.shape + ({d.out_dim},), got {tuple(g.shape)}")
        keep.append(gc)
        r = {"tok_table": (torch.empty if n else torch.zeros)((d.tok_rows, d.token_dim), dtype=dt, device=dev),   # written once by the call
             "byte_table": torch.zeros((d.byte_rows, d.byte_dim), dtype=torch.float32, device=dev),
             "weight": torch.zeros((d.out_dim, d.token_dim + bpt * d.byte_dim), dtype=torch.float32, device=dev)}
        res.append(r)
        gr.slot[j].grad_out, gr.slot[j].d_tok, gr.slot[j].d_byte, gr.slot[j].d_weight = capi.ptr(gc), capi.ptr(r["tok_table"]), capi.ptr(r["byte_table"]), capi.ptr(r["weight"])
        if norm_out:
            xo = _contig(outs[j], dt, f"outs[{j}]")
            rn = _contig(row_rnorms[j], torch.float32, f"row_rnorms[{j}]")
            if xo.numel() != n * d.out_dim or rn.numel() != n:
                raise ValueError(f"outs[{j}] / row_rnorms[{j}] are not the forward's")
            keep += [xo, rn]
            d.slot[j].out, d.slot[j].out_row_rnorm = capi.ptr(xo), capi.ptr(rn)
    if n == 0 or all(g is None for g in grad_outs):
        return res
    _bind_token_order(gr, keep, token_order, n, d.tok_rows, dev)
    _launch(dev, d, capi.lib.mot_value_mix_bwd, C.byref(gr), ws_bytes=lambda p: capi.lib.mot_value_mix_workspace_bytes(p, 1))
    return res


class _ValueMixFn(torch.autograd.Function):
    """Autograd node of value_mix: one mot_value_mix_fwd call forward, one mot_value_mix_bwd call backward for every slot's two
    tables and weight.  Saved: the tokens, the byte ids, the parameters and, with norm_out, the outputs and 4 bytes per token and
    slot of row factors; u is gathered again.  The token order comes from the cache the fused front-end uses."""

    @staticmethod
    def forward(ctx, tokens, kw, *params):
        n = len(params) // 3
        tt, bt, ws = params[:n], params[n:2 * n], params[2 * n:]
        outs, ids, rns = _value_mix_fwd(tokens, [t.detach() for t in tt], [t.detach() for t in bt], [t.detach() for t in ws], save=True, **kw)
        ctx.order = _token_orders.get(tokens, tt[0].shape[0]) if _HOIST_SORT and tokens.numel() else None
        ctx.n, ctx.normed = n, rns is not None
        ctx.kw = dict(bpt=kw["bpt"], norm_out=kw.get("norm_out", True), eps=kw.get("eps"))
        ctx.save_for_backward(tokens, ids, *params, *(outs if rns is not None else ()), *(rns or ()))
        ctx.set_materialize_grads(False)   # an output nothing depends on arrives as None and its slot is skipped
        return outs

    @staticmethod
    def backward(ctx, *grads):
        n = ctx.n
        tokens, ids, *rest = ctx.saved_tensors
        tt, bt, ws = rest[:n], rest[n:2 * n], rest[2 * n:3 * n]
        outs, rns = (rest[3 * n:4 * n], rest[4 * n:5 * n]) if ctx.normed else (None, None)
        gs = [g if any(ctx.needs_input_grad[2 + k * n + j] for k in range(3)) else None for j, g in enumerate(grads[:n])]
        if all(g is None for g in gs):
            return (None,) * (2 + 3 * n)
        res = value_mix_backward(gs, tokens, [t.detach() for t in tt], [t.detach() for t in bt], [t.detach() for t in ws], ids=ids,
                                 outs=None if outs is None else [o.detach() for o in outs], row_rnorms=rns,
                                 token_order=_ready_order(ctx.order, tokens.device), **ctx.kw)
        pick = lambda k, ps: tuple(None if r is None else _grad_like(r[k], p) for r, p in zip(res, ps))   # bf16: the fp32 sums rounded once
        return (None, None, *pick("tok_table", tt), *pick("byte_table", bt), *pick("weight", ws))


def value_mix(tokens: torch.Tensor, tok_tables, byte_tables, weights, *, bpt: int, ids: torch.Tensor | None = None, ttb: torch.Tensor | None = None,
              pull: str | None = None, pad_byte: int = 456, eot_byte: int = 457, norm_out: bool = True, eps: float | None = None) -> tuple:
    """The mixture-of-tokenizers value embeddings of modded-nanogpt/runs/9_mot-in_mot-valemb.py:310-313 (runs 3 and 6 alike):
    for each of the 1..4 slots j, ``ve_j = norm(cat(tok_tables[j][tokens], byte_tables[j][ids[:, 0]], ..., byte_tables[j][ids[:,
    bpt-1]]) @ weights[j].T)`` with weights[j] (out_dim, token_dim + bpt*byte_dim) in nn.Linear layout, no bias; float32 or
    bfloat16 throughout (bf16: fp32 sums, rounded where the reference's bf16 run rounds: F.linear's result, then the normalised
    row).  tokens (B, T) or (T,); the byte ids are in per-token order (.., T*bpt), given as `ids` (int64) or made once for all
    slots from the token->byte table `ttb` (+ `pull` = "left" | "right" | None) inside the call.  `eps` None is the float32 epsilon
    for both dtypes.  Returns a tuple of ``tokens.shape + (out_dim,)`` tensors through ONE autograd node: its backward is one call
    for all slots over one token order, and every token table's gradient is written once, in the table's dtype."""
    tt, bt, ws = list(tok_tables), list(byte_tables), list(weights)
    capi.require_device(tokens, *tt, *bt, *ws, ids, ttb)
    kw = dict(bpt=bpt, ids=ids, ttb=ttb, pull=pull, pad_byte=pad_byte, eot_byte=eot_byte, norm_out=norm_out, eps=eps)
    if torch.is_grad_enabled() and any(p.requires_grad for p in (*tt, *bt, *ws)):
        _value_mix_desc(tokens, tt, bt, ws, bpt, norm_out, eps, "value_mix")   # shape and dtype errors before the node exists
        return tuple(_ValueMixFn.apply(tokens, kw, *tt, *bt, *ws))
    return _value_mix_fwd(tokens, tt, bt, ws, **kw)[0]


# ------------------------------------------------------------------------------------------------
# the three input streams of modded-nanogpt/runs/71081_mot-in_toks-valemb.py:302-304, 315:
# x0t = norm(E_t[tok]), x0b = cat_k norm(E_b[id_k]), x = s_t x0t + s_b x0b, all from one call
# ------------------------------------------------------------------------------------------------
_SPLIT_X0_OUTS = ("x0t", "x0b", "x")


def _split_x0_scalar(s, what):
    """A one-element float32 tensor (0-dim, (1,), or a one-element slice of a longer parameter): the kernel reads it where it lives."""
    if not isinstance(s, torch.Tensor) or s.numel() != 1:
        raise ValueError(f"{what} must be a one-element tensor on the device (the run's scalars[-1] / scalars[-2]); the host never reads it")
    if s.dtype != torch.float32:
        raise TypeError(f"{what}: expected torch.float32, got {s.dtype}")
    return s.reshape(1)   # a view of one element is always contiguous


def _split_x0_desc(tokens, tok_table, byte_table, scale_tok, scale_byte, bpt, eps, what):
    """The descriptor's problem part, checked: tokens (B, T) int32 contiguous, a (tok_rows, model_dim) and a (byte_rows, byte_dim)
    table of one dtype, the two scalars.  What the library does not build (model_dim != bpt * byte_dim, ...) is left to its refusal."""
    if tok_table.dtype != byte_table.dtype:
        raise TypeError(f"{what}: the byte table is {byte_table.dtype} but the token table is {tok_table.dtype}: all tensors share one dtype")
    capi.dtype_code(tok_table.dtype)
    if tok_table.ndim != 2 or byte_table.ndim != 2:
        raise ValueError(f"{what}: tables must be 2-D, got {tuple(tok_table.shape)} and {tuple(byte_table.shape)}")
    tok = _tokens_2d(tokens, f"{what}: tokens must be (B, T) or (T,)")
    tt, bt = _table(tok_table, f"{what}: token table"), _table(byte_table, f"{what}: byte table")
    st, sb = _split_x0_scalar(scale_tok, f"{what}: scale_tok"), _split_x0_scalar(scale_byte, f"{what}: scale_byte")
    d = capi.MotSplitX0Desc()
    d.struct_size = C.sizeof(capi.MotSplitX0Desc)
    d.dtype = capi.dtype_code(tt.dtype)
    d.n_rows, d.tokens_per_row, d.bpt = tok.shape[0], tok.shape[1], int(bpt)
    d.model_dim, d.byte_dim = tt.shape[1], bt.shape[1]
    d.tokens, d.tok_table, d.tok_rows, d.byte_table, d.byte_rows = capi.ptr(tok), capi.ptr(tt), tt.shape[0], capi.ptr(bt), bt.shape[0]
    d.scale_tok, d.scale_byte = capi.ptr(st), capi.ptr(sb)
    d.eps = float(eps or 0.0)
    return d, tok, [tok, tt, bt, st, sb]


def _split_x0_want(want):
    want = tuple(want)
    if not want or any(w not in _SPLIT_X0_OUTS for w in want) or len(set(want)) != len(want):
        raise ValueError(f"split_x0: want must name one to three of {_SPLIT_X0_OUTS}, each once, got {want}")
    return want


@torch.compiler.disable
def _split_x0_fwd(tokens, tok_table, byte_table, scale_tok, scale_byte, *, bpt, ids=None, ttb=None, pull="left", pad_byte=456, eot_byte=457,
                  eps=None, want=_SPLIT_X0_OUTS, save=False, return_ids=False, counters=None):
    """One mot_splitx_fwd call.  Returns ({name: tensor} for the wanted outputs, ids_used): with `save` the ids the byte table was read
    with (the given ones, or those made from `ttb`), which the backward wants.  With `return_ids` (ids from `ttb` only) it returns
    (outs, ids_padded, ids_pulled) instead, the int64 tensors the kernel wrote; `counters` is an int64[4] device tensor the kernel
    adds its statistics to, as in embed_mix."""
    dev = capi.require_device(tokens, tok_table, byte_table, scale_tok, scale_byte, ids, ttb)
    want = _split_x0_want(want)
    d, tok, keep = _split_x0_desc(tokens, tok_table, byte_table, scale_tok, scale_byte, bpt, eps, "split_x0")
    B, T = tok.shape
    outs = {w: torch.empty(tuple(tokens.shape) + (d.model_dim,), dtype=tok_table.dtype, device=dev) for w in want}
    if return_ids and ttb is None and ids is not None:
        raise ValueError("split_x0: return_ids needs the token->byte table (ttb)")
    ids_used = _bind_byte_ids(d, keep, B=B, T=T, bpt=bpt, ids=ids, ttb=ttb, pull=pull, what="split_x0", ids_what=_IDS_PER_TOKEN.format("split_x0"))
    if ttb is not None and (save or return_ids):
        ids_used = _new_ids(B, T, bpt, dev)
        d.out_ids_pulled = capi.ptr(ids_used)   # without a pull the "pulled" ids are the table's rows
    if ttb is not None and return_ids:
        ids_padded = _new_ids(B, T, bpt, dev)
        d.out_ids_padded = capi.ptr(ids_padded)
    d.pad_byte, d.eot_byte = int(pad_byte), int(eot_byte)
    _bind_counters(d, counters, dev)
    if B * T == 0:   # an empty batch: nothing to launch
        return (outs, ids_padded, ids_used) if return_ids else (outs, ids_used)
    d.out_x0t, d.out_x0b, d.out_x = (capi.ptr(outs.get(w)) for w in _SPLIT_X0_OUTS)
    _launch(dev, d, capi.lib.mot_splitx_fwd, ws_bytes=lambda p: capi.lib.mot_splitx_workspace_bytes(p, 0))
    if return_ids:
        return outs, ids_padded, ids_used
    return outs, (ids_used if save else None)


@torch.compiler.disable
def split_x0_backward(grad_x0t, grad_x0b, grad_x, tokens, tok_table, byte_table, scale_tok, scale_byte, *, bpt, ids, eps=None, token_order=None,
                      want_grads=("tok_table", "byte_table", "scale_tok", "scale_byte"), out=None, into=None) -> dict:
    """One call of mot_splitx_bwd.  Each of the three upstream gradients ``tokens.shape + (model_dim,)`` may be None (zero; it is
    passed to the library as NULL), at least one is given.  Returns a dict with the entries named in `want_grads`:
    "tok_table" in the TABLES' dtype, every element written exactly once by the call (fp32 sums in ascending position order rounded
    once, +0 rows for absent ids, the same bits on every run, with or without `token_order`; `out` names a buffer to write it INTO,
    whatever it held); "byte_table" fp32, accumulated (+=) into `into` or into a fresh zeroed tensor (LDS fixed-point sums flushed
    with float atomics); "scale_tok" and "scale_byte" fp32 one-element tensors, written, the same bits on every run.  Nothing of the
    forward is needed but the byte `ids` it used."""
    gs = [grad_x0t, grad_x0b, grad_x]
    dev = capi.require_device(tokens, tok_table, byte_table, scale_tok, scale_byte, ids, token_order, out, into, *[g for g in gs if g is not None])
    if all(g is None for g in gs):
        raise ValueError("split_x0_backward: grad_x0t, grad_x0b and grad_x are all None")
    d, tok, keep = _split_x0_desc(tokens, tok_table, byte_table, scale_tok, scale_byte, bpt, eps, "split_x0_backward")
    _bind_byte_ids(d, keep, B=d.n_rows, T=d.tokens_per_row, bpt=bpt, ids=ids, ttb=None, pull=None, what="split_x0_backward",
                   ids_what=_IDS_PER_TOKEN.format("split_x0_backward"))
    n, dt = tok.numel(), tok_table.dtype
    gr = capi.MotSplitX0Grads()
    gr.struct_size = C.sizeof(capi.MotSplitX0Grads)
    for name, g in zip(("grad_x0t", "grad_x0b", "grad_x"), gs):
        if g is None:
            continue
        gc = _contig(g, dt, name)
        if gc.numel() != n * d.model_dim:
            raise ValueError(f"{name} must be tokens.shape + ({d.model_dim},), got {tuple(g.shape)}")
        keep.append(gc)
        setattr(gr, name, capi.ptr(gc))
    res = {}
    if "tok_table" in want_grads:
        r = out
        if r is None:
            r = (torch.empty if n else torch.zeros)((d.tok_rows, d.model_dim), dtype=dt, device=dev)   # written once by the call
        elif r.dtype != dt or tuple(r.shape) != (d.tok_rows, d.model_dim) or not r.is_contiguous():
            raise ValueError(f"out must be a contiguous {dt} tensor of the token table's shape")
        elif n == 0:
            r.zero_()
        res["tok_table"], gr.d_tok_table = r, capi.ptr(r)
    if "byte_table" in want_grads:
        r = into if into is not None else torch.zeros((d.byte_rows, d.byte_dim), dtype=torch.float32, device=dev)
        if r.dtype != torch.float32 or tuple(r.shape) != (d.byte_rows, d.byte_dim) or not r.is_contiguous():
            raise ValueError("into must be a contiguous float32 tensor of the byte table's shape")
        res["byte_table"], gr.d_byte_table = r, capi.ptr(r)
    if "scale_tok" in want_grads or "scale_byte" in want_grads:
        sc = torch.zeros(2, dtype=torch.float32, device=dev)   # (an empty batch launches nothing: zeros)
        if "scale_tok" in want_grads:
            res["scale_tok"], gr.d_scale_tok = sc[0:1], sc.data_ptr()
        if "scale_byte" in want_grads:
            res["scale_byte"], gr.d_scale_byte = sc[1:2], sc.data_ptr() + 4
        keep.append(sc)
    if n == 0 or not res:
        return res
    _bind_token_order(gr, keep, token_order, n, d.tok_rows, dev)
    _launch(dev, d, capi.lib.mot_splitx_bwd, C.byref(gr), ws_bytes=lambda p: capi.lib.mot_splitx_workspace_bytes(p, 1))
    return res


class _SplitX0Fn(torch.autograd.Function):
    """Autograd node of split_x0: one mot_splitx_fwd call forward, one mot_splitx_bwd call backward for the two tables and the two
    scalars.  Saved: the tokens, the byte ids, the tables and the scalars; every row is gathered and normalised again.  The token
    order comes from the cache the fused front-end uses."""

    @staticmethod
    def forward(ctx, tokens, kw, tok_table, byte_table, scale_tok, scale_byte):
        outs, ids = _split_x0_fwd(tokens, tok_table.detach(), byte_table.detach(), scale_tok.detach(), scale_byte.detach(), save=True, **kw)
        ctx.order = _token_orders.get(tokens, tok_table.shape[0]) if _HOIST_SORT and tokens.numel() and tok_table.requires_grad else None
        ctx.want = _split_x0_want(kw.get("want", _SPLIT_X0_OUTS))
        ctx.kw = dict(bpt=kw["bpt"], eps=kw.get("eps"))
        ctx.save_for_backward(tokens, ids, tok_table, byte_table, scale_tok, scale_byte)
        ctx.set_materialize_grads(False)   # an output nothing depends on arrives as None and goes to the library as NULL
        return tuple(outs[w] for w in ctx.want)

    @staticmethod
    def backward(ctx, *grads):
        tokens, ids, tok_table, byte_table, scale_tok, scale_byte = ctx.saved_tensors
        g = dict(zip(ctx.want, grads))
        names = [n for j, n in enumerate(("tok_table", "byte_table", "scale_tok", "scale_byte")) if ctx.needs_input_grad[2 + j]]
        if all(v is None for v in g.values()) or not names:
            return (None,) * 6
        r = split_x0_backward(g.get("x0t"), g.get("x0b"), g.get("x"), tokens, tok_table.detach(), byte_table.detach(), scale_tok.detach(),
                              scale_byte.detach(), ids=ids, token_order=_ready_order(ctx.order, tokens.device), want_grads=names, **ctx.kw)
        pick = lambda k, p: _grad_like(r.get(k), p)   # bf16 byte table: the fp32 sums rounded once
        return (None, None, pick("tok_table", tok_table), pick("byte_table", byte_table), pick("scale_tok", scale_tok), pick("scale_byte", scale_byte))


def split_x0(tokens: torch.Tensor, tok_table: torch.Tensor, byte_table: torch.Tensor, scale_tok: torch.Tensor, scale_byte: torch.Tensor, *, bpt: int,
             ids: torch.Tensor | None = None, ttb: torch.Tensor | None = None, pull: str | None = "left", pad_byte: int = 456, eot_byte: int = 457,
             eps: float | None = None, want=_SPLIT_X0_OUTS) -> tuple:
    """The three input streams of modded-nanogpt/runs/71081_mot-in_toks-valemb.py:302-304, 315 in one launch:
    ``x0t = norm(tok_table[tokens])``, ``x0b = cat_k norm(byte_table[ids[:, k]])`` (each byte row normalised over byte_dim BEFORE the
    cat) and ``x = x0t * scale_tok + x0b * scale_byte`` (no outer norm), with model_dim = bpt * byte_dim; float32 or bfloat16 throughout
    (bf16: fp32 arithmetic, rounded where the reference's eager bf16 run rounds).  tokens (B, T) or (T,); the byte ids are in per-token
    order (.., T*bpt), given as `ids` (int64) or made inside the kernel from the token->byte table `ttb` (+ `pull` = "left" | "right" |
    None).  `scale_tok` / `scale_byte` are one-element float32 tensors on the device (the run's ``scalars[-1]`` / ``scalars[-2]``; a
    slice of a longer parameter works, and its gradient flows back into that parameter).  `eps` None is the float32 epsilon for both
    dtypes.  Returns the tensors named in `want`, in that order, each ``tokens.shape + (model_dim,)``, through ONE autograd node whose
    backward is one call: the token table's gradient is written once in the table's dtype with the same bits on every run."""
    capi.require_device(tokens, tok_table, byte_table, scale_tok, scale_byte, ids, ttb)
    want = _split_x0_want(want)
    kw = dict(bpt=int(bpt), ids=ids, ttb=ttb, pull=pull, pad_byte=pad_byte, eot_byte=eot_byte, eps=eps, want=want)
    params = (tok_table, byte_table, scale_tok, scale_byte)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        _split_x0_desc(tokens, *params, bpt, eps, "split_x0")   # shape and dtype errors before the node exists
        return tuple(_SplitX0Fn.apply(tokens, kw, *params))
    outs, _ = _split_x0_fwd(tokens, *params, **kw)
    return tuple(outs[w] for w in want)
