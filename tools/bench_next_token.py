"""The generation step: fused (functional.next_token) vs the eager restatement of inference/inference.py:420-444 on the same GPU
(F.linear on the last position, / temperature, topk, sort, cumsum, scatter, softmax, multinomial), at temperature 0.8, top_k 50,
top_p 0.9.  One JSON line per shape:
    B 1, 8 and 64 at 128 256 x 2048 in fp32 and bf16; B 1 and 64 at 50 304 x 768 in fp32
with, per shape: the fused call and the eager step (device events around `--inner` calls, median of `--reps` warmed repetitions, in
microseconds a call); the fused call without cuts (plain sampling) and greedy; F.linear alone; the kernels of the fused call alone
(mean device time from torch.profiler over a few calls: the skinny product or, above 16 rows, the rows kernel and the heads' product,
and the row pass); and the product's floor vocab * model_dim * element size / 8 TB/s.

    python tools/bench_next_token.py [--out FILE] [--reps N] [--inner N]
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
HBM_BYTES_PER_S = 8.0e12
T, TOP_K, TOP_P = 0.8, 50, 0.9
KERNELS = ("nexttoken_skinny", "nexttoken_rows_in", "nexttoken_row", "gemm_rows")   # names (plain or mangled) are matched in this order
CASES = [(V, D, B, dt) for V, D in ((128256, 2048),) for dt in (torch.float32, torch.bfloat16) for B in (1, 8, 64)] + \
        [(50304, 768, B, torch.float32) for B in (1, 64)]


def eager_step(hidden, w):
    """lines 420-444 with the wrapper's lm_head in front"""
    logits = F.linear(hidden[:, -1, :], w) / T
    remove = logits < torch.topk(logits, TOP_K)[0][..., -1, None]
    logits[remove] = float("-inf")
    sorted_logits, sorted_indices = torch.sort(logits, descending=True)
    cum = torch.cumsum(torch.softmax(sorted_logits, dim=-1), dim=-1)
    sorted_remove = cum > TOP_P
    sorted_remove[..., 1:] = sorted_remove[..., :-1].clone()
    sorted_remove[..., 0] = 0
    remove = sorted_remove.scatter(1, sorted_indices, sorted_remove)
    logits[remove] = float("-inf")
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs.float(), num_samples=1)


def timed_us(f, reps, inner):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            f()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1000.0 / inner)
    ts.sort()
    return round(ts[len(ts) // 2], 2)


def kernel_us(f, calls=5):
    """mean device time per call of every kernel f launches, by kernel name; None with the reason when the profiler gives none"""
    from torch.profiler import ProfilerActivity, profile
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                f()
            torch.cuda.synchronize()
        got = {}
        for e in prof.events():
            t = float(getattr(e, "device_time", 0.0) or 0.0)
            if t > 0:
                name = next((k for k in KERNELS if k in e.name), e.name.split("<")[0].split("(")[0].split()[-1])
                got[name] = got.get(name, 0.0) + t
        return ({k: round(v / calls, 2) for k, v in got.items()} or None), (None if got else "the profiler returned no kernel times")
    except Exception as e:   # optional; the reason goes into the record
        return None, f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    lines = []
    with torch.no_grad():
        for V, D, B, dt in CASES:
            g = torch.Generator(device=DEV).manual_seed(1)
            hidden = torch.randn(B, 4, D, device=DEV, generator=g).to(dt)
            w = (torch.randn(V, D, device=DEV, generator=g) * 3.0 / D ** 0.5).to(dt)
            u = torch.rand(B, device=DEV, generator=g)
            last = hidden[:, -1, :]
            e = w.element_size()
            rec = {"vocab": V, "model_dim": D, "rows": B, "dtype": str(dt).split(".")[1], "temperature": T, "top_k": TOP_K, "top_p": TOP_P,
                   "product_floor_us": round(V * D * e / HBM_BYTES_PER_S * 1e6, 1)}
            fused = lambda: mot.next_token(last, w, temperature=T, top_k=TOP_K, top_p=TOP_P, u=u)
            rec["fused_us"] = timed_us(fused, args.reps, args.inner)
            rec["fused_no_cuts_us"] = timed_us(lambda: mot.next_token(last, w, temperature=T, u=u), args.reps, args.inner)
            rec["fused_greedy_us"] = timed_us(lambda: mot.next_token(last, w, greedy=True), args.reps, args.inner)
            rec["eager_us"] = timed_us(lambda: eager_step(hidden, w), args.reps, args.inner)
            rec["f_linear_us"] = timed_us(lambda: F.linear(last, w), args.reps, args.inner)
            rec["speedup"] = round(rec["eager_us"] / rec["fused_us"], 2)
            ks, why = kernel_us(fused)
            rec["fused_kernels_us"] = ks
            if ks is None:
                rec["fused_kernels_unmeasured"] = why
            else:
                prod = sum(v for k, v in ks.items() if "nexttoken_row" != k)   # everything but the row pass: the product side
                rec["product_us"], rec["row_pass_us"] = round(prod, 2), ks.get("nexttoken_row")
                rec["product_share_of_floor"] = round(rec["product_floor_us"] / prod, 3) if prod else None
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            del hidden, w
            mot.functional.release_workspaces()
            torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
