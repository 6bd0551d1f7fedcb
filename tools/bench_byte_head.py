"""Byte output head: fused (functional.byte_head_loss) vs the eager torch restatement (tests/byte_head_ref.py's expressions) on the
same GPU.  One JSON line per case: copy / split x fp32 / bf16 at 8x1024 and 64x1024 tokens, model_dim 1024, bpt 16, n_layer_out 1.
Times are device events over warmed repetitions (median ms); peak extra memory is max_memory_allocated above the inputs.
`bound_us` is what the case is judged against: the MFMA time of its forward (+ backward) products at the dense peak, and for
split also the transcendental issue time of 3 per logit at 8 cycles per wave instruction (1024 SIMDs at 2.4 GHz).

    python tools/bench_byte_head.py [--out FILE] [--reps N]
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


def eager(x, w, t, method, bpt, L):
    h = x.repeat_interleave(bpt, dim=-2) if method == "copy" else x.reshape(*x.shape[:-2], x.shape[-2] * bpt, x.shape[-1] // bpt)
    for _ in range(L):
        h = h + F.rms_norm(h, (h.size(-1),))
    logits = F.linear(F.rms_norm(h, (h.size(-1),)), w.type_as(h))
    z = 30 * torch.sigmoid(logits.float() / 7.5)
    return F.cross_entropy(z.view(-1, z.size(-1)), t.view(-1))


def fused(x, w, t, method, bpt, L):
    return mot.byte_head_loss(x, w, t, method=method, bytes_per_token=bpt, n_layer_out=L)


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

    for _ in range(3):
        fwd_bwd()
    torch.cuda.synchronize()
    x.grad = w.grad = None
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
    args = ap.parse_args()
    D, bpt, L = 1024, 16, 1
    lines = []
    for tokens in (8 * 1024, 64 * 1024):
        for method in ("copy", "split"):
            for dt_name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
                K = D if method == "copy" else D // bpt
                g = torch.Generator(device=DEV).manual_seed(1)
                x = torch.randn(tokens // 1024, 1024, D, device=DEV, generator=g).to(dt).requires_grad_(True)
                w = ((torch.rand(512, K, device=DEV, generator=g) * 2 - 1) * 0.5 * (3 / K) ** 0.5).requires_grad_(True)
                t = torch.randint(0, 458, (tokens // 1024, 1024 * bpt), device=DEV, generator=g)
                rec = {"case": f"{method}_{dt_name}_{tokens}", "method": method, "dtype": dt_name, "tokens": tokens, "model_dim": D,
                       "bpt": bpt, "n_layer_out": L}
                fw, fb, pk = measure(lambda a, b, c: fused(a, b, c, method, bpt, L), x, w, t, args.reps)
                rec.update(fused_fwd_ms=round(fw, 4), fused_fwd_bwd_ms=round(fb, 4), fused_peak_extra_mib=round(pk / 2 ** 20, 1))
                fw, fb, pk = measure(lambda a, b, c: eager(a, b, c, method, bpt, L), x, w, t, args.reps)
                rec.update(eager_fwd_ms=round(fw, 4), eager_fwd_bwd_ms=round(fb, 4), eager_peak_extra_mib=round(pk / 2 ** 20, 1))
                rec["speedup_fwd_bwd"] = round(rec["eager_fwd_bwd_ms"] / rec["fused_fwd_bwd_ms"], 2)
                rows = tokens * (bpt if method == "split" else 1)
                flops_fwd = 2.0 * rows * 512 * K
                mfma_us = flops_fwd / (PEAK_TFLOPS[dt_name] * 1e12) * 1e6
                rec["bound"] = {"mfma_fwd_us": round(mfma_us, 2), "mfma_fwd_bwd_us": round(4 * mfma_us, 2)}   # bwd: s again, G W, G^T x
                if method == "split":
                    logits = rows * 512
                    rec["bound"]["transcendental_fwd_us"] = round(logits * 3 / 64 * 8 / (SIMDS * CLOCK_HZ) * 1e6, 2)
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
                del x, w, t
                torch.cuda.empty_cache()
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
