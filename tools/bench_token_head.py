"""Token-level output head: fused (functional.token_head_loss) vs the eager torch restatement (tests/token_head_ref.py's expressions)
on the same GPU.  One JSON line per case: 65 536 rows, 50 304 classes, model_dim 768 and 1024, fp32 and bf16, both softcaps at
model_dim 768.  Times are device events over warmed repetitions (median ms), forward only (no_grad) and forward + backward to finished
gradients; peak extra memory is max_memory_allocated above the inputs, the library's
workspace released first so that it is counted.  `floor` is what the case is judged against: three products
of 2 N V D FLOP at the rates the launchers reach, and one read and one write of e V bytes per row for the row
pass at the HBM rate.  --rows / --reps shorten a run (the eager side needs 50 to 90 GB at the full size).

    python tools/bench_token_head.py [--out FILE] [--reps N] [--rows N] [--no-eager]
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
import mixture_of_tokenizers_amd as mot  # noqa: E402

DEV = torch.device("cuda", 0)
V = 50304
LAUNCHER_TFLOPS = {"fp32": 110.0, "bf16": 740.0}   # what gemm_rows / gemm_rows_bf16 reach at large shapes
HBM_TBS = 4.0                                      # a streaming kernel's achievable rate (tools/hbm_ceilings.py)


def eager(x, w, t, kind):
    logits = F.linear(F.rms_norm(x, (x.size(-1),)), w.type_as(x)).float()
    z = 30 * torch.sigmoid(logits / 7.5) if kind == "sigmoid30" else 15 * logits * torch.rsqrt(logits.square() + 225)
    return F.cross_entropy(z, t)


def fused(x, w, t, kind):
    return mot.token_head_loss(x, w, t, softcap=kind)


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


def measure(run, x, w, t, reps):
    def fwd():
        with torch.no_grad():
            run(x, w, t)

    def fwd_bwd():
        x.grad = w.grad = None
        run(x, w, t).backward()

    for _ in range(2):
        fwd_bwd()
    torch.cuda.synchronize()
    x.grad = w.grad = None
    mot.functional.release_workspaces()   # the library's workspace (a chunk's logits, u, the transposed W) counts as extra memory
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fwd_bwd()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return timed(fwd, reps), timed(fwd_bwd, reps), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    N = args.rows
    lines = []
    for D, kind in ((768, "sigmoid30"), (768, "rsqrt15"), (1024, "sigmoid30")):
        for dt_name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
            g = torch.Generator(device=DEV).manual_seed(1)
            x = torch.randn(N, D, device=DEV, generator=g).to(dt).requires_grad_(True)
            w = ((torch.rand(V, D, device=DEV, generator=g) * 2 - 1) * 0.5 * (3 / D) ** 0.5).requires_grad_(True)
            t = torch.randint(0, 50257, (N,), device=DEV, generator=g)
            rec = {"case": f"{kind}_{dt_name}_D{D}_N{N}", "softcap": kind, "dtype": dt_name, "rows": N, "model_dim": D, "vocab": V}
            fw, fb, pk = measure(lambda a, b, c: fused(a, b, c, kind), x, w, t, args.reps)
            rec.update(fused_fwd_ms=round(fw, 3), fused_fwd_bwd_ms=round(fb, 3), fused_peak_extra_mib=round(pk / 2 ** 20, 1))
            mot.functional.release_workspaces()
            torch.cuda.empty_cache()
            if not args.no_eager:
                try:
                    fw, fb, pk = measure(lambda a, b, c: eager(a, b, c, kind), x, w, t, args.reps)
                    rec.update(eager_fwd_ms=round(fw, 3), eager_fwd_bwd_ms=round(fb, 3), eager_peak_extra_mib=round(pk / 2 ** 20, 1))
                    rec["speedup_fwd_bwd"] = round(rec["eager_fwd_bwd_ms"] / rec["fused_fwd_bwd_ms"], 2)
                    rec["memory_ratio"] = round(rec["eager_peak_extra_mib"] / rec["fused_peak_extra_mib"], 1)
                except torch.OutOfMemoryError as e:
                    rec["eager_error"] = str(e).split(".")[0]
            product_ms = 2.0 * N * V * D / (LAUNCHER_TFLOPS[dt_name] * 1e12) * 1e3
            row_pass_ms = N * V * (4 if dt_name == "fp32" else 2) / (HBM_TBS * 1e12) * 1e3
            rec["floor"] = {"product_ms": round(product_ms, 3), "fwd_ms": round(product_ms + row_pass_ms, 3),
                            "fwd_bwd_ms": round(3 * product_ms + 2 * row_pass_ms, 3)}
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del x, w, t
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
