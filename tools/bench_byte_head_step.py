"""Byte output head, split mode: the one-call step (functional.byte_head_loss(one_call=True) -> mot_byte_head_step) vs the two-call
path (mot_byte_head_fwd / _bwd) in the same process vs the eager torch restatement, forward + backward, on the same GPU.
One JSON line per case: fp32 / bf16 at 8x1024 and 64x1024 tokens, model_dim 1024, bpt 16 (1 M byte rows of K = 64 at the larger
size), n_layer_out 1.  Times are device events over warmed repetitions (median ms, and the min / max of the repetitions as the
spread); peak extra memory is max_memory_allocated above the inputs.  A dtype the one-call step refuses is recorded as refused.
`floor_ms` is DESIGN section 7's: the four products at the dense MFMA peak and the transcendental issue time, whichever is larger.

    python tools/bench_byte_head_step.py [--out FILE] [--reps N] [--only one_call|two_call|eager] [--dtypes bf16,fp32]
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
PEAK_TFLOPS = {"fp32": 157.3, "bf16": 2516.6}   # dense MFMA peaks (MI355X_MICROARCH.md)
SIMDS, CLOCK_HZ = 1024, 2.4e9


def eager(x, w, t, bpt, L):
    h = x.reshape(*x.shape[:-2], x.shape[-2] * bpt, x.shape[-1] // bpt)
    for _ in range(L):
        h = h + F.rms_norm(h, (h.size(-1),))
    logits = F.linear(F.rms_norm(h, (h.size(-1),)), w.type_as(h))
    z = 30 * torch.sigmoid(logits.float() / 7.5)
    return F.cross_entropy(z.view(-1, z.size(-1)), t.view(-1))


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
    return ts[len(ts) // 2], ts[0], ts[-1]


def measure(run, x, w, t, reps):
    def fwd_bwd():
        x.grad = w.grad = None
        run(x, w, t).backward()

    for _ in range(3):
        fwd_bwd()
    torch.cuda.synchronize()
    x.grad = w.grad = None
    mot.functional.release_workspaces()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fwd_bwd()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    fwd_bwd()
    torch.cuda.synchronize()
    med, lo, hi = timed(fwd_bwd, reps)
    return {"fwd_bwd_ms": round(med, 4), "min_ms": round(lo, 4), "max_ms": round(hi, 4), "peak_extra_mib": round(peak / 2 ** 20, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", default=None, choices=("one_call", "two_call", "eager"))
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--tokens", default="8192,65536")
    args = ap.parse_args()
    D, bpt, L = 1024, 16, 1
    K = D // bpt
    paths = {
        "one_call": lambda a, b, c: mot.byte_head_loss(a, b, c, method="split", bytes_per_token=bpt, n_layer_out=L, one_call=True),
        "two_call": lambda a, b, c: mot.byte_head_loss(a, b, c, method="split", bytes_per_token=bpt, n_layer_out=L),
        "eager": lambda a, b, c: eager(a, b, c, bpt, L),
    }
    if args.only:
        paths = {args.only: paths[args.only]}
    lines = []
    for tokens in (int(v) for v in args.tokens.split(",")):
        for dt_name in args.dtypes.split(","):
            dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[dt_name]
            g = torch.Generator(device=DEV).manual_seed(1)
            x = torch.randn(tokens // 1024, 1024, D, device=DEV, generator=g).to(dt).requires_grad_(True)
            w = ((torch.rand(512, K, device=DEV, generator=g) * 2 - 1) * 0.5 * (3 / K) ** 0.5).requires_grad_(True)
            t = torch.randint(0, 458, (tokens // 1024, 1024 * bpt), device=DEV, generator=g)
            rows = tokens * bpt
            rec = {"case": f"split_{dt_name}_{tokens}", "dtype": dt_name, "tokens": tokens, "model_dim": D, "bpt": bpt, "n_layer_out": L}
            for name, run in paths.items():
                try:
                    rec[name] = measure(run, x, w, t, args.reps)
                except NotImplementedError as e:
                    rec[name] = {"refused": str(e)}
            if "fwd_bwd_ms" in rec.get("one_call", {}) and "fwd_bwd_ms" in rec.get("two_call", {}):
                rec["two_call_over_one_call"] = round(rec["two_call"]["fwd_bwd_ms"] / rec["one_call"]["fwd_bwd_ms"], 2)
            mfma_ms = 4 * 2.0 * rows * 512 * K / (PEAK_TFLOPS[dt_name] * 1e12) * 1e3   # s (twice), G W, G^T x
            trans_ms = 2 * rows * 512 * 3 / 64 * 8 / (SIMDS * CLOCK_HZ) * 1e3             # 3 per logit, forward and backward
            rec["floor_ms"] = round(max(mfma_ms, trans_ms), 3)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del x, w, t
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
