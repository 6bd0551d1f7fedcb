"""Byte self-attention layer: the HIP call (functional.byte_self_attn) vs the same layer in eager torch on the same GPU, and the
three-part split of a run-1.3 model front (gather + norm, attention layer, concat + linear + norm).

The eager side is the plain-torch restatement of tests/byte_self_attn_ref.py in float32 with the band taken by chunks of 512 queries
(each chunk sees its own keys and the window before it; nothing of the L x L score matrix outside the band is formed).
Shapes: the per-GPU shape of run 1.3 (B 8, L 16 384 = 1024 tokens x 16 bytes, window 128, D 48, one head) and D 768 (six heads).
Times are device events over warmed repetitions (median ms); peak extra memory is max_memory_allocated above the inputs over one
forward + backward.  `floor` is what the attention is judged against: the two attention products of the forward, 4 W 128 FLOP per
head and byte position, at the fp32 matrix peak, and the bytes of the input and output rows (and of the q, k, v round trip through
HBM, which this version takes) at the HBM peak.  One JSON line per record.

    python tools/bench_byte_self_attn.py [--out FILE] [--reps N] [--profile-only]

--profile-only runs a few fused forward + backward steps at the first shape and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats`.
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import byte_self_attn_ref as br  # noqa: E402
import mixture_of_tokenizers_amd as mot  # noqa: E402
from mixture_of_tokenizers_amd import modules as M  # noqa: E402

DEV = torch.device("cuda", 0)
PEAK_FP32_TFLOPS, PEAK_HBM_TBS = 157.3, 8.0   # MI355X_MICROARCH.md


def timed(f, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def measure(run, leaves, g, reps):
    def fwd():
        with torch.no_grad():
            run()

    def fwd_bwd():
        for t in leaves:
            t.grad = None
        run().backward(g)

    for _ in range(3):
        fwd_bwd()
    torch.cuda.synchronize()
    for t in leaves:
        t.grad = None
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fwd_bwd()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return timed(fwd, reps), timed(fwd_bwd, reps), peak


def layer_case(D, B, L, bpt, window, reps, profile_only=False):
    x, w, pw, lam, g = (t.to(DEV) for t in br.make_inputs(1, D, B, L))
    cos, sin = (t.to(DEV) for t in br.rotary_tables(L))
    leaves = [t.requires_grad_(True) for t in (x, w, pw, lam)]
    kw = dict(bpt=bpt, window=window, block_causal=False)
    fused = lambda: mot.functional.byte_self_attn(x, w, pw, lam, cos, sin, **kw)
    eager = lambda: br.byte_self_attn(x, w, pw, lam, cos, sin, chunk=512, **kw)
    if profile_only:
        for _ in range(5):
            for t in leaves:
                t.grad = None
            fused().backward(g)
        torch.cuda.synchronize()
        return None
    H = br.n_heads(D)
    rec = {"record": "layer", "B": B, "L": L, "D": D, "heads": H, "bpt": bpt, "window": window, "mask": "causal",
           "eager": "restatement, float32, band by chunks of 512 queries"}
    fw, fb, pk = measure(fused, leaves, g, reps)
    rec.update(fused_fwd_ms=round(fw, 4), fused_fwd_bwd_ms=round(fb, 4), fused_peak_extra_mib=round(pk / 2 ** 20, 1))
    fw, fb, pk = measure(eager, leaves, g, reps)
    rec.update(eager_fwd_ms=round(fw, 4), eager_fwd_bwd_ms=round(fb, 4), eager_peak_extra_mib=round(pk / 2 ** 20, 1))
    rec["speedup_fwd"] = round(rec["eager_fwd_ms"] / rec["fused_fwd_ms"], 2)
    rec["speedup_fwd_bwd"] = round(rec["eager_fwd_bwd_ms"] / rec["fused_fwd_bwd_ms"], 2)
    n = B * L
    attn_flop = 4.0 * window * 128 * H * n
    proj_flop = 2.0 * n * D * 4 * H * 128          # x qkv_w^T and y c_proj^T
    io_bytes = 2.0 * n * D * 4
    qkv_bytes = 2.0 * n * 3 * H * 128 * 4          # written by the projection, read by the attention kernel
    rec["floor"] = {"attn_gflop_fwd": round(attn_flop / 1e9, 2), "attn_mfma_fwd_us": round(attn_flop / (PEAK_FP32_TFLOPS * 1e12) * 1e6, 1),
                    "proj_mfma_fwd_us": round(proj_flop / (PEAK_FP32_TFLOPS * 1e12) * 1e6, 1),
                    "io_rows_mb": round(io_bytes / 1e6, 1), "io_rows_us": round(io_bytes / (PEAK_HBM_TBS * 1e12) * 1e6, 1),
                    "qkv_round_trip_mb": round(qkv_bytes / 1e6, 1), "qkv_round_trip_us": round(qkv_bytes / (PEAK_HBM_TBS * 1e12) * 1e6, 1)}
    return rec


def front_split(reps):
    """run 1.3: model_dim 1024, byte_dim 48, token_dim 256, B 8 x T 1024, bpt 16, window 8 tokens.  Each part is timed on its own, its
    inputs detached, forward and forward + backward."""
    B, T, bpt, vocab = 8, 1024, 16, 50304
    bp = M.ByteHyperparameters(bytes_per_token=bpt, byte_mixin_method="concat", use_byte_self_attn=True, sliding_window_tokens=8)
    dims = M.ModelDims(model_dim=1024, byte_dim=48, token_dim=256)
    torch.manual_seed(0)
    emb, mixin = M.FlexibleEmbedding(dims, vocab, bp).to(DEV), M.ByteMixin(dims, T, bp).to(DEV)
    with torch.no_grad():
        mixin.mixin.attention.attention.c_proj.reset_parameters()
    gen = torch.Generator(device=DEV).manual_seed(2)
    toks = torch.randint(0, vocab, (B, T), device=DEV, generator=gen, dtype=torch.int32)
    ids = torch.randint(0, 458, (B, T * bpt), device=DEV, generator=gen)
    n = lambda t: F.rms_norm(t, (t.size(-1),))
    gather = lambda: (n(F.embedding(toks.long(), emb.embed_tokens.weight)), n(F.embedding(ids, emb.embed_bytes.weight)))
    with torch.no_grad():
        te, be = gather()
    te_l, be_l = te.clone().requires_grad_(True), be.clone().requires_grad_(True)
    layer = mixin.mixin.attention
    with torch.no_grad():
        ba = layer(be)
    ba_l = ba.clone().requires_grad_(True)
    contract = lambda: n(mixin.mixin.mixin(torch.cat([te_l, ba_l.reshape(B, T, bpt * 48)], dim=-1)))
    g_be, g_x = torch.randn_like(be), torch.randn(B, T, 1024, device=DEV)
    params = list(emb.parameters()) + list(mixin.parameters())
    rec = {"record": "run_1_3_front_split", "B": B, "T": T, "bpt": bpt, "model_dim": 1024, "byte_dim": 48, "token_dim": 256,
           "gather_and_contraction": "plain torch ops", "attention": "mot_byte_self_attn_fwd / _bwd"}
    parts = {
        "gather_norm": (lambda: gather()[1], params, g_be),            # the byte rows (the token rows ride along in the forward)
        "attention": (lambda: layer(be_l), params + [be_l], g_be),
        "contraction_norm": (contract, params + [te_l, ba_l], g_x),
    }
    for name, (run, leaves, g) in parts.items():
        fw, fb, _ = measure(run, leaves, g, reps)
        rec[f"{name}_fwd_ms"], rec[f"{name}_fwd_bwd_ms"] = round(fw, 4), round(fb, 4)
    whole = lambda: mixin(*emb(toks, ids, ids))
    fw, fb, pk = measure(whole, params, g_x, reps)
    rec.update(whole_fwd_ms=round(fw, 4), whole_fwd_bwd_ms=round(fb, 4), whole_peak_extra_mib=round(pk / 2 ** 20, 1))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile-only", action="store_true")
    args = ap.parse_args()
    if args.profile_only:
        layer_case(48, 8, 16384, 16, 128, args.reps, profile_only=True)
        return
    lines = []
    for D in (48, 768):
        lines.append(json.dumps(layer_case(D, 8, 16384, 16, 128, args.reps)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    lines.append(json.dumps(front_split(args.reps)))
    print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
