"""Token value embeddings (functional.value_embeds; scaled-pre-train/train_gpt.py:566, 600 and modded-nanogpt/runs/
71_*_toks-valemb.py:247, 303): one gather launch and the write-once table gradients against what a caller had before, all in one
process on the same tokens, the variants alternated repetition by repetition:

  (a) eager torch: three F.embedding forward + backward() (one embedding_dense_backward per table);
  (b) three embed_mix(mode="noop", norm_tok=False) calls sharing one token order: fp32 atomic row-adds into dense, pre-zeroed
      fp32 buffers, rounded to the parameter's dtype by autograd.  (b) is timed twice per repetition; the distance between its two
      medians is the spread against which "not slower than (b)" is judged.

Shapes: 65 536 tokens (64 x 1024, the per-GPU step of both training scripts) at dim 1024, and the headline batch of 524 288 tokens
at dim 768; vocabulary 50 257, three tables, bf16 and fp32; ids FineWeb-shaped (golden_inputs.fineweb_like_tokens, seed 12345:
bench.py's generator and seed) and uniform.
Times are device events over warmed repetitions (median ms, with [min, max]).  Algorithmic bytes: forward N n 2 D e; backward
N n D e read plus Vt n D e written; `hbm_frac` is bytes / time over the 8 TB/s peak.  One JSON line per record.

    python tools/bench_value_embeds.py [--out FILE] [--reps N] [--quick] [--fused-only]
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
import golden_inputs as gi  # noqa: E402
import mixture_of_tokenizers_amd as mot  # noqa: E402

DEV = torch.device("cuda", 0)
PEAK_HBM_TBS = 8.0   # MI355X_MICROARCH.md
VOCAB, TABLES = gi.GPT2_VOCAB, 3


def timed_alternating(variants: dict, reps: int, warm: int = 3) -> dict:
    """{name: (median, min, max) ms}: every variant warmed, then one timing of each per repetition, in turn"""
    for f in variants.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in variants}
    for _ in range(reps):
        for k, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = (v[len(v) // 2], v[0], v[-1])
    return out


def put(rec, key, t, nbytes=None):
    med, lo, hi = t
    rec[key + "_ms"] = round(med, 4)
    rec[key + "_min_max_ms"] = [round(lo, 4), round(hi, 4)]
    if nbytes:
        rec[key + "_hbm_frac"] = round(nbytes / (med * 1e-3) / (PEAK_HBM_TBS * 1e12), 4)


def case(N, D, dtype, ids, reps, fused_only=False):
    e = 2 if dtype == torch.bfloat16 else 4
    g = torch.Generator(device=DEV).manual_seed(12345)
    tables = [torch.randn((VOCAB, D), generator=g, device=DEV).to(dtype) for _ in range(TABLES)]
    toks = torch.from_numpy(gi.fineweb_like_tokens(12345, 1, N, vocab=VOCAB, uniform=ids == "uniform").reshape(-1)).to(DEV)
    gouts = [torch.randn((N, D), generator=g, device=DEV).to(dtype) for _ in range(TABLES)]
    fwd_bytes = N * TABLES * 2 * D * e
    bwd_bytes = N * TABLES * D * e + VOCAB * TABLES * D * e
    rec = {"record": "value_embeds", "tokens": N, "dim": D, "vocab": VOCAB, "tables": TABLES, "dtype": str(dtype).replace("torch.", ""), "ids": ids,
           "reps": reps, "top_id_share": round(float(torch.bincount(toks).max()) / N, 4),
           "alg_bytes": {"fwd": fwd_bytes, "bwd": bwd_bytes, "fwd_bwd": fwd_bytes + bwd_bytes}}
    fused = lambda tabs: mot.value_embeds(toks, tabs)
    eager = lambda tabs: [F.embedding(toks, t) for t in tabs]
    noop3 = lambda tabs: [mot.embed_mix(toks, t, mode="noop", norm_tok=False).reshape(N, D) for t in tabs]
    with torch.no_grad():
        variants = {"fused_fwd": lambda: fused(tables)}
        if not fused_only:
            variants.update(a_eager_fwd=lambda: eager(tables), b_noop3_fwd=lambda: noop3(tables))
            rec["fwd_equal_eager"] = all(torch.equal(a, b) for a, b in zip(fused(tables), eager(tables)))
        for k, t in timed_alternating(variants, reps).items():
            put(rec, k, t, fwd_bytes)
    torch.cuda.empty_cache()

    leaves = [t.clone().requires_grad_(True) for t in tables]

    def fwd_bwd(run):
        def f():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(list(run(leaves)), gouts)
        return f
    det = [t.detach() for t in leaves]
    order = mot.functional.token_order(toks, VOCAB)
    variants = {"fused_fwd_bwd": fwd_bwd(fused), "fused_bwd_given_order": lambda: mot.functional.value_embeds_backward(gouts, toks, det, token_order=order),
                "fused_bwd_own_order": lambda: mot.functional.value_embeds_backward(gouts, toks, det)}
    if not fused_only:
        variants.update(b_noop3_fwd_bwd=fwd_bwd(noop3), a_eager_fwd_bwd=fwd_bwd(eager), b_noop3_fwd_bwd_again=fwd_bwd(noop3))
    res = timed_alternating(variants, reps)
    for k, t in res.items():
        put(rec, k, t, {"fused_fwd_bwd": fwd_bytes + bwd_bytes, "fused_bwd_given_order": bwd_bytes, "fused_bwd_own_order": bwd_bytes}.get(k))
    if not fused_only:
        b1, b2 = rec["b_noop3_fwd_bwd_ms"], rec["b_noop3_fwd_bwd_again_ms"]
        rec["b_spread_ms"] = round(abs(b1 - b2), 4)
        rec["speedup_fwd_bwd_vs_a"] = round(rec["a_eager_fwd_bwd_ms"] / rec["fused_fwd_bwd_ms"], 2)
        rec["speedup_fwd_bwd_vs_b"] = round(min(b1, b2) / rec["fused_fwd_bwd_ms"], 2)
        rec["not_slower_than_b"] = rec["fused_fwd_bwd_ms"] <= min(b1, b2) + rec["b_spread_ms"]
    mot.check_status()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the 65 536-token step in bf16 with FineWeb-shaped ids only")
    ap.add_argument("--fused-only", action="store_true", help="leave (a) and (b) out: for a kernel trace of the library's own launches")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    shapes = [(65536, 1024, torch.bfloat16, "fineweb")]
    if not args.quick:
        shapes += [(65536, 1024, torch.float32, "fineweb"), (65536, 1024, torch.bfloat16, "uniform"), (65536, 1024, torch.float32, "uniform"),
                   (524288, 768, torch.bfloat16, "fineweb"), (524288, 768, torch.float32, "fineweb"), (524288, 768, torch.bfloat16, "uniform")]
    lines = []
    for N, D, dtype, ids in shapes:
        lines.append(json.dumps(case(N, D, dtype, ids, args.reps, args.fused_only)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
        mot.functional.release_workspaces()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
