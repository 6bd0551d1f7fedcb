"""Evaluation form of the output heads (functional.token_head_eval / byte_head_eval) against (a) the no-grad loss call at the same
shape and (b) eager torch producing the same five outputs (loss, row_loss, pred, rank, counts), on the same GPU.  One JSON line per
case: the token-level head at 65 536 rows x 768 and x 1024 over 50 304 classes, both softcaps, fp32 and bf16; the byte head in copy
and split at 64 x 1024 tokens, model_dim 1024, 16 bytes per token, fp32 and bf16.

The expectation under test: the evaluation reads no logit the loss call does not read and writes 12 bytes per row, so it should cost
what the loss call costs, within that call's own run-to-run spread.  So the two are timed in `--rounds` alternating rounds (device
events over `--reps` warmed repetitions, the median of a round), and a case reports every round, the loss call's spread over the
rounds ((max - min) / median) and the ratio of the medians.  Peak extra memory is max_memory_allocated above the inputs with the
library's workspace released first, so that it is counted.  --loss-only times the loss call alone, and --root imports the library
from another checkout (a built parent commit, for its spread); --rows / --tokens shorten a run.

    python tools/bench_head_eval.py [--out FILE] [--rounds N] [--reps N] [--rows N] [--tokens N] [--no-eager] [--loss-only] [--root DIR] [--tag NAME]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

DEV = torch.device("cuda", 0)
V, BYTE_V, BPT = 50304, 512, 16


def softcap(l, kind):
    return 30 * torch.sigmoid(l / 7.5) if kind == "sigmoid30" else 15 * l * torch.rsqrt(l.square() + 225)


def five_outputs(logits, z, t, per):
    """What the evaluation returns, from materialised logits [M, V] (as the product stored them) and capped logits z (fp32)."""
    row_loss = F.cross_entropy(z, t, reduction="none")
    pred = logits.argmax(1).int()
    rank = (logits > logits.gather(1, t[:, None])).sum(1).int()
    hit = pred == t
    counts = [torch.tensor(t.numel(), device=t.device), hit.sum()]
    if per:
        counts.append(hit.reshape(-1, per).all(1).sum())
    return row_loss.mean(), row_loss, pred, rank, torch.stack(counts)


def eager_token(x, w, t, kind):
    logits = F.linear(F.rms_norm(x, (x.size(-1),)), w.type_as(x))
    return five_outputs(logits, softcap(logits.float(), kind), t, None)


def eager_byte(x, w, t, method, L):
    h = x.repeat_interleave(BPT, dim=0) if method == "copy" else x.reshape(-1, x.shape[-1] // BPT)
    for _ in range(L):
        h = h + F.rms_norm(h, (h.size(-1),))
    logits = F.linear(F.rms_norm(h, (h.size(-1),)), w.type_as(h)).float()
    return five_outputs(logits, softcap(logits, "sigmoid30"), t, BPT)


def timed(f, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def peak_extra(mot, f):
    mot.functional.release_workspaces()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return round(peak / 2 ** 20, 1)


def measure(mot, rec, calls, args):
    """calls: name -> callable, `loss` first.  Alternating rounds; the medians of the rounds, the loss call's spread, the ratios."""
    with torch.no_grad():
        for name, f in calls.items():
            try:
                rec[f"{name}_peak_extra_mib"] = peak_extra(mot, f)   # also the warm-up of this shape
                f()
            except torch.OutOfMemoryError as e:
                rec[f"{name}_error"] = str(e).split(".")[0]
        live = {k: f for k, f in calls.items() if f"{k}_error" not in rec}
        rounds = {k: [] for k in live}
        for _ in range(args.rounds):
            for name, f in live.items():
                rounds[name].append(round(timed(f, max(2, args.reps // 4) if name == "eager" else args.reps), 4))
    for name, ts in rounds.items():
        rec[f"{name}_ms_rounds"] = ts
        rec[f"{name}_ms"] = round(statistics.median(ts), 4)
    ls = rounds["loss"]
    rec["loss_spread"] = round((max(ls) - min(ls)) / statistics.median(ls), 4)
    if "eval" in rounds:
        rec["eval_over_loss"] = round(rec["eval_ms"] / rec["loss_ms"], 4)
        rec["eval_within_spread"] = bool(rec["eval_ms"] <= max(ls))
    if "eager" in rounds and "eval" in rounds:
        rec["eager_over_eval"] = round(rec["eager_ms"] / rec["eval_ms"], 2)
        rec["memory_ratio"] = round(rec["eager_peak_extra_mib"] / max(rec["eval_peak_extra_mib"], 0.1), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=8)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--tokens", type=int, default=64 * 1024)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--loss-only", action="store_true")
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[1]), help="the checkout whose library is timed")
    ap.add_argument("--tag", default="this")
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import mixture_of_tokenizers_amd as mot
    assert Path(mot.__file__).resolve().is_relative_to(Path(args.root).resolve()), mot.__file__
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    def calls_of(loss, evaluate, eager):
        calls = {"loss": loss}
        if not args.loss_only:
            calls["eval"] = evaluate
            if not args.no_eager:
                calls["eager"] = eager
        return calls

    N = args.rows
    for D in (768, 1024):
        for kind in ("sigmoid30", "rsqrt15"):
            for dt_name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
                g = torch.Generator(device=DEV).manual_seed(1)
                x = torch.randn(N, D, device=DEV, generator=g).to(dt)
                w = (torch.rand(V, D, device=DEV, generator=g) * 2 - 1) * 0.5 * (3 / D) ** 0.5
                t = torch.randint(0, 50257, (N,), device=DEV, generator=g)
                rec = {"tag": args.tag, "head": "token", "case": f"token_{kind}_{dt_name}_D{D}_N{N}", "softcap": kind, "dtype": dt_name, "rows": N,
                       "model_dim": D, "vocab": V}
                measure(mot, rec, calls_of(lambda: mot.token_head_loss(x, w, t, softcap=kind),
                                           lambda: mot.token_head_eval(x, w, t, softcap=kind),
                                           lambda: eager_token(x, w, t, kind)), args)
                emit(rec)
                del x, w, t
                torch.cuda.empty_cache()
    T, D, L = args.tokens, 1024, 1
    for method in ("copy", "split"):
        for dt_name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            g = torch.Generator(device=DEV).manual_seed(2)
            K = D if method == "copy" else D // BPT
            x = torch.randn(T, D, device=DEV, generator=g).to(dt)
            w = (torch.rand(BYTE_V, K, device=DEV, generator=g) * 2 - 1) * 0.5 * (3 / K) ** 0.5
            t = torch.randint(0, 458, (T * BPT,), device=DEV, generator=g)
            rec = {"tag": args.tag, "head": "byte", "case": f"byte_{method}_{dt_name}_D{D}_T{T}", "method": method, "dtype": dt_name, "tokens": T,
                   "model_dim": D, "bpt": BPT, "n_layer_out": L, "vocab": BYTE_V}
            kw = dict(method=method, bytes_per_token=BPT, n_layer_out=L)
            measure(mot, rec, calls_of(lambda: mot.byte_head_loss(x, w, t, **kw), lambda: mot.byte_head_eval(x, w, t, **kw),
                                       lambda: eager_byte(x, w, t, method, L)), args)
            emit(rec)
            del x, w, t
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
