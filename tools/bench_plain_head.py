"""Plain cross-entropy head: fused (functional.plain_head_loss) vs eager torch (F.rms_norm, F.linear, .float(), F.cross_entropy with
ignore_index) on the same GPU.  One JSON line per case:
    fp32, 50 304 x 768, 65 536 rows, every row kept and 1 row in 16 kept (the scored windows of mathblations)
    bf16 and fp32, 128 256 x 2048, 16 384 rows, a tenth of the targets -100, no norm (the inference wrapper)
and one line that times functional.token_head_loss(softcap="rsqrt15") at 50 304 x 768 in the same process: the plain head differs
from it by the row maximum and the divisor read on the device, so the ratio of the two should be close to 1.
Beside them the compacted call (max_kept, functional.plain_head_loss(..., max_kept=...)) on the same inputs, in the same process and
with the same timing: 1 row in 16 kept with max_kept = the exact count and twice the count (the cost of a loose bound), the bf16
inference case with the exact count, and every row kept with max_kept = rows (the overhead of index, gather and scatter when nothing
is dropped).  Each compacted line carries the un-compacted call (max_kept=None), eager torch as the reference writes it (full logits,
then the slice) and eager torch that gathers the kept rows first, and the index pass's own time (the three kernels' mean durations
from torch.profiler over a few forward calls; null with the reason when the profiler gives no kernel times).
Times are device events over warmed repetitions (median ms), forward only (no_grad) and forward + backward to finished gradients;
peak extra memory is max_memory_allocated above the inputs, the library's workspace released first so that it is counted.
--rows-scale shortens a run.

    python tools/bench_plain_head.py [--out FILE] [--reps N] [--rows-scale F] [--no-eager] [--compact-only] [--no-compact]
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
CASES = [  # name, dtype, vocab, model_dim, rows, norm_in, share of rows kept
    ("mathblations_all_kept", torch.float32, 50304, 768, 65536, True, 1.0),
    ("mathblations_1_in_16_kept", torch.float32, 50304, 768, 65536, True, 1 / 16),
    ("inference_bf16", torch.bfloat16, 128256, 2048, 16384, False, 0.9),
    ("inference_fp32", torch.float32, 128256, 2048, 16384, False, 0.9),
]
# compacted runs of a case: (label, max_kept as a multiple of the exact kept count; None: max_kept = rows)
COMPACT = {
    "mathblations_1_in_16_kept": [("exact", 1), ("loose_2x", 2)],
    "inference_bf16": [("exact", 1)],
    "mathblations_all_kept": [("rows", None)],
}
INDEX_KERNELS = ("compact_count", "compact_scan", "compact_write")


def eager(x, w, t, norm_in):
    h = F.rms_norm(x, (x.size(-1),)) if norm_in else x
    return F.cross_entropy(F.linear(h, w.type_as(x)).float(), t, ignore_index=-100)


def eager_slice(x, w, t, norm_in):
    """as the reference writes it (model.py:337-338, slice_logits_and_targets): the logits of every row, then the kept rows of them"""
    h = F.rms_norm(x, (x.size(-1),)) if norm_in else x
    logits = F.linear(h, w.type_as(x)).float()
    keep = t != -100
    return F.cross_entropy(logits[keep], t[keep])


def eager_gather_first(x, w, t, norm_in):
    keep = t != -100
    h = x[keep]
    h = F.rms_norm(h, (h.size(-1),)) if norm_in else h
    return F.cross_entropy(F.linear(h, w.type_as(x)).float(), t[keep])


def index_pass_us(run, x, w, t, calls=5):
    """mean device time of one index pass (its three kernels), from torch.profiler over `calls` forward calls"""
    from torch.profiler import ProfilerActivity, profile
    try:
        with torch.no_grad(), profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(calls):
                run(x, w, t)
            torch.cuda.synchronize()
        got = {k: [] for k in INDEX_KERNELS}
        for e in prof.events():
            for k in INDEX_KERNELS:
                if k in e.name:
                    got[k].append(float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)))
        if any(len(v) != calls for v in got.values()):
            return None, f"profiler saw {[len(v) for v in got.values()]} launches of the index kernels, expected {calls} each"
        return {k: round(sum(v) / calls, 2) for k, v in got.items()}, None
    except Exception as e:   # the measurement is optional; the reason goes into the record
        return None, f"{type(e).__name__}: {e}"


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
    mot.functional.release_workspaces()   # the library's workspace counts as extra memory
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
    ap.add_argument("--rows-scale", type=float, default=1.0)
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--compact-only", action="store_true", help="only the cases that have compacted runs")
    ap.add_argument("--no-compact", action="store_true", help="only the un-compacted lines")
    args = ap.parse_args()
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for name, dt, V, D, rows, norm_in, kept in CASES:
        if args.compact_only and name not in COMPACT:
            continue
        N = max(256, int(rows * args.rows_scale) // 256 * 256)
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(N, D, device=DEV, generator=g).to(dt).requires_grad_(True)
        w = ((torch.rand(V, D, device=DEV, generator=g) * 2 - 1) * 0.5 * (3 / D) ** 0.5).requires_grad_(True)
        t = torch.randint(0, V, (N,), device=DEV, generator=g)
        t[torch.rand(N, device=DEV, generator=g) >= kept] = -100
        rec = {"case": name, "dtype": str(dt).split(".")[1], "rows": N, "kept": int((t != -100).sum()), "model_dim": D, "vocab": V, "norm_in": norm_in}
        fw, fb, pk = measure(lambda a, b, c: mot.plain_head_loss(a, b, c, norm_in=norm_in), x, w, t, args.reps)
        rec.update(fused_fwd_ms=round(fw, 3), fused_fwd_bwd_ms=round(fb, 3), fused_peak_extra_mib=round(pk / 2 ** 20, 1))
        if name == "mathblations_all_kept":   # the capped head on the same operands, in the same process
            cf, cb, _ = measure(lambda a, b, c: mot.token_head_loss(a, b, c, softcap="rsqrt15"), x, w, t.clamp_min(0), args.reps)
            rec.update(token_head_rsqrt15_fwd_ms=round(cf, 3), token_head_rsqrt15_fwd_bwd_ms=round(cb, 3),
                       ratio_to_token_head_fwd=round(fw / cf, 3), ratio_to_token_head_fwd_bwd=round(fb / cb, 3))
        mot.functional.release_workspaces()
        torch.cuda.empty_cache()
        if not args.no_eager:
            try:
                fw, fb, pk = measure(lambda a, b, c: eager(a, b, c, norm_in), x, w, t, args.reps)
                rec.update(eager_fwd_ms=round(fw, 3), eager_fwd_bwd_ms=round(fb, 3), eager_peak_extra_mib=round(pk / 2 ** 20, 1))
                rec["speedup_fwd_bwd"] = round(rec["eager_fwd_bwd_ms"] / rec["fused_fwd_bwd_ms"], 2)
                rec["memory_ratio"] = round(rec["eager_peak_extra_mib"] / rec["fused_peak_extra_mib"], 1)
            except torch.OutOfMemoryError as e:
                rec["eager_error"] = str(e).split(".")[0]
        emit(rec)
        for label, factor in ([] if args.no_compact else COMPACT.get(name, [])):
            mk = N if factor is None else min(N, factor * rec["kept"])
            run = lambda a, b, c: mot.plain_head_loss(a, b, c, norm_in=norm_in, max_kept=mk)
            crec = {"case": f"{name}_compact_{label}", "dtype": rec["dtype"], "rows": N, "kept": rec["kept"], "max_kept": mk, "model_dim": D, "vocab": V,
                    "norm_in": norm_in, "uncompacted_fwd_ms": rec["fused_fwd_ms"], "uncompacted_fwd_bwd_ms": rec["fused_fwd_bwd_ms"],
                    "uncompacted_peak_extra_mib": rec["fused_peak_extra_mib"]}
            fw, fb, pk = measure(run, x, w, t, args.reps)
            crec.update(compact_fwd_ms=round(fw, 3), compact_fwd_bwd_ms=round(fb, 3), compact_peak_extra_mib=round(pk / 2 ** 20, 1),
                        speedup_vs_uncompacted_fwd_bwd=round(rec["fused_fwd_bwd_ms"] / fb, 2))
            us, why = index_pass_us(run, x, w, t)
            crec["index_pass_us"] = us
            if us is not None:
                crec["index_pass_total_us"] = round(sum(us.values()), 2)
            else:
                crec["index_pass_unmeasured"] = why
            mot.functional.release_workspaces()
            torch.cuda.empty_cache()
            if not args.no_eager and label != "loose_2x":   # the eager paths do not depend on the bound
                for key, f in (("eager_slice", eager_slice), ("eager_gather_first", eager_gather_first)):
                    try:
                        fw, fb, pk = measure(lambda a, b, c: f(a, b, c, norm_in), x, w, t, args.reps)
                        crec.update({f"{key}_fwd_ms": round(fw, 3), f"{key}_fwd_bwd_ms": round(fb, 3), f"{key}_peak_extra_mib": round(pk / 2 ** 20, 1)})
                        crec[f"speedup_vs_{key}_fwd_bwd"] = round(fb / crec["compact_fwd_bwd_ms"], 2)
                    except torch.OutOfMemoryError as e:
                        crec[f"{key}_error"] = str(e).split(".")[0]
                    torch.cuda.empty_cache()
            emit(crec)
        del x, w, t
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
