"""The fused front-end with the write-once backward (functional.embed_mix(write_once=True); mot_embed_mix_bwd_once) against the path
it is an alternative to, all in one process on the same tensors, the variants alternated repetition by repetition.  What is timed is
forward + backward through autograd up to a finished .grad in the parameters' dtype:

  (b1), (b2)  embed_mix as it was: the backward adds into zeroed fp32 buffers with float atomics and, for bf16 tables, rounds them
              (the zero fill and the rounding pass are inside the timing: the node needs them).  Timed TWICE, as two variants of the
              rotation, so that the spread between two medians of the same thing is on record;
  (c)         embed_mix(write_once=True).

Shapes: 65 536 tokens at 1024 / 64 / 16 (run 71's step) and 524 288 tokens at 768 / 48 / 16 (the headline batch); fp32 and bf16;
token ids FineWeb-shaped and uniform (golden_inputs.fineweb_like_tokens, seed 12345), byte ids uniform over the 458 byte rows;
modes "sum" (run 71: norm_out) and "concat" (512 / 32 / 16, norm_out; model_dim 1024).  Times are device events, the median of
`--reps` warmed repetitions with [min, max].  "c not slower than b" is read against (b)'s own spread: c's median is at most the
larger of the two (b) medians plus their difference.  Peak extra memory is torch's peak allocated bytes over one forward + backward
beyond what was allocated before it (workspaces included: they are dropped before each measurement).  One JSON line per record.

    python tools/bench_embed_mix_once.py [--out FILE] [--reps N] [--quick] [--trace-only]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import golden_inputs as gi  # noqa: E402
import mixture_of_tokenizers_amd as mot  # noqa: E402

DEV = torch.device("cuda", 0)
VOCAB, BYTE_ROWS = gi.GPT2_VOCAB, gi.BYTE_VOCAB


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
        out[k] = (round(v[len(v) // 2], 4), round(v[0], 4), round(v[-1], 4))
    return out


def peak_extra_mb(f) -> float:
    """peak allocated bytes during f() beyond the bytes allocated before it, workspaces and caches dropped first"""
    mot.functional.release_workspaces()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    f()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(DEV) - base) / 2 ** 20, 1)


def setup(N, mode, Dt, Db, bpt, dtype, ids_kind):
    g = torch.Generator(device=DEV).manual_seed(12345)
    rnd = lambda *shape: torch.randn(shape, generator=g, device=DEV).to(dtype)
    Dm = Dt + bpt * Db if mode == "concat" else Dt
    Et, Eb, gout = rnd(VOCAB, Dt), rnd(BYTE_ROWS, Db), rnd(1, N, Dm)
    toks = torch.from_numpy(gi.fineweb_like_tokens(12345, 1, N, vocab=VOCAB, uniform=ids_kind == "uniform")).to(DEV)
    ids = torch.randint(0, BYTE_ROWS, (1, N * bpt), generator=g, device=DEV, dtype=torch.int64)
    leaves = [Et.requires_grad_(True), Eb.requires_grad_(True)]

    def fwd_bwd(write_once):
        def f():
            for t in leaves:
                t.grad = None
            x = mot.embed_mix(toks, leaves[0], leaves[1], mode=mode, bpt=bpt, ids_a=ids, norm_out=True, write_once=write_once)
            x.backward(gout)
        return f
    return leaves, fwd_bwd


def case(N, mode, Dt, Db, bpt, dtype, ids_kind, reps):
    leaves, fwd_bwd = setup(N, mode, Dt, Db, bpt, dtype, ids_kind)
    rec = {"record": "embed_mix_once", "tokens": N, "mode": mode, "tok_dim": Dt, "byte_dim": Db, "bpt": bpt, "vocab": VOCAB,
           "dtype": str(dtype).replace("torch.", ""), "ids": ids_kind, "reps": reps}
    old, new = fwd_bwd(False), fwd_bwd(True)
    old()
    ref = [t.grad.float().clone() for t in leaves]
    new()
    assert all(t.grad.dtype == dtype for t in leaves)
    rec["grad_max_diff_vs_b"] = [float((t.grad.float() - r).abs().max()) for t, r in zip(leaves, ref)]
    rec["grad_max_abs"] = [float(r.abs().max()) for r in ref]
    first = [t.grad.clone() for t in leaves]
    new()
    rec["c_same_bits_twice"] = all(torch.equal(t.grad, f) for t, f in zip(leaves, first))
    del ref, first
    times = timed_alternating({"b1_atomic_fwd_bwd": old, "c_write_once_fwd_bwd": new, "b2_atomic_fwd_bwd": old}, reps)
    for k, (med, lo, hi) in times.items():
        rec[k + "_ms"], rec[k + "_min_max_ms"] = med, [lo, hi]
    b1, b2, c = times["b1_atomic_fwd_bwd"][0], times["b2_atomic_fwd_bwd"][0], times["c_write_once_fwd_bwd"][0]
    rec["b_spread_ms"] = round(abs(b1 - b2), 4)
    rec["ratio_b_over_c"] = round(min(b1, b2) / c, 3)
    rec["c_not_slower_than_b"] = c <= max(b1, b2) + abs(b1 - b2)
    rec["c_faster_than_b"] = times["c_write_once_fwd_bwd"][2] < min(times["b1_atomic_fwd_bwd"][1], times["b2_atomic_fwd_bwd"][1])
    rec["b_peak_extra_mb"], rec["c_peak_extra_mb"] = peak_extra_mb(old), peak_extra_mb(new)
    d = mot._capi.MotEmbedMixDesc()   # the shape only: what the size queries look at
    d.struct_size, d.dtype, d.mode = ctypes.sizeof(d), mot._capi.dtype_code(dtype), mot.functional._MODES[mode]
    d.n_rows, d.tokens_per_row, d.bpt, d.id_source = 1, N, bpt, mot._capi.IDS_GIVEN
    d.tok_rows, d.byte_rows, d.tok_dim, d.byte_dim, d.norm_out = VOCAB, BYTE_ROWS, Dt, Db, 1
    d.model_dim = Dt + bpt * Db if mode == "concat" else Dt
    rec["b_bwd_workspace_mb"] = round(mot._capi.lib.mot_embed_mix_bwd_workspace_bytes(ctypes.byref(d)) / 2 ** 20, 1)
    rec["c_bwd_workspace_mb"] = round(mot._capi.lib.mot_embed_mix_bwd_once_workspace_bytes(ctypes.byref(d)) / 2 ** 20, 1)
    mot.check_status()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="run 71's step in bf16, FineWeb-shaped ids, mode sum only")
    ap.add_argument("--trace-only", action="store_true",
                    help="no timing: three steps of each path at the headline batch in bf16, for a kernel trace taken from outside")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    if args.trace_only:
        _, fwd_bwd = setup(524288, "sum", 768, 48, 16, torch.bfloat16, "fineweb")
        for f in (fwd_bwd(False), fwd_bwd(True)):
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        return
    shapes = [(65536, "sum", 1024, 64, 16)]
    if not args.quick:
        shapes += [(524288, "sum", 768, 48, 16), (65536, "concat", 512, 32, 16), (524288, "concat", 512, 32, 16)]
    lines = []
    for N, mode, Dt, Db, bpt in shapes:
        for dtype in (torch.bfloat16,) if args.quick else (torch.float32, torch.bfloat16):
            for ids_kind in ("fineweb",) if args.quick else ("fineweb", "uniform"):
                lines.append(json.dumps(case(N, mode, Dt, Db, bpt, dtype, ids_kind, args.reps)))
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
                mot.functional.release_workspaces()
                if args.out:   # after every case: a later one that runs out of time loses nothing
                    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
                    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
