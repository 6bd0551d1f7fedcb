"""Run 71081's three streams (functional.split_x0; modded-nanogpt/runs/71081_mot-in_toks-valemb.py:302-304, 315): one forward and one
backward call for x0t, x0b and x against what a caller had before, all in one process on the same tensors, the variants alternated
repetition by repetition:

  (a) eager torch of the four lines on the same device: F.embedding, F.rms_norm, the cat, the weighted sum;
  (b) the best composition the library offered before split_x0: embed_mix(mode="sum", norm_tok, norm_byte, scalars, norm_out=False)
      for x, plus embed_mix(mode="noop", norm_tok=True) for x0t, plus torch gather / rms_norm / reshape for x0b;
  (c) a plain fill_ of the three outputs: the floor of a forward that is three quarters writes.

Shapes: the run's own step (1 x 65 536 tokens at 1024 / 64 / 16) and the headline batch (256 x 2048 at 768 / 48 / 16), fp32 and bf16,
GPT-2 vocabulary, 458 byte rows.  Token ids FineWeb-shaped (golden_inputs.fineweb_like_tokens, seed 12345), byte ids uniform over the
byte vocabulary.  Times are device events, the median of `--reps` warmed repetitions with [min, max]: "faster than (b)" means the
one call's [min, max] lies below (b)'s [min, max].  Peak extra memory is torch's peak allocated bytes over one forward + backward
beyond what was allocated before it (workspaces included: they are dropped before each measurement).  One JSON line per record.

    python tools/bench_split_x0.py [--out FILE] [--reps N] [--quick]
"""
from __future__ import annotations

import argparse
import ctypes
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
VOCAB, BYTE_ROWS = gi.GPT2_VOCAB, gi.BYTE_VOCAB
F32_EPS = 2.0 ** -23


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


def case(B, T, D, Db, bpt, dtype, reps):
    N = B * T
    g = torch.Generator(device=DEV).manual_seed(12345)
    rnd = lambda *shape: torch.randn(shape, generator=g, device=DEV).to(dtype)
    Et, Eb = rnd(VOCAB, D), rnd(BYTE_ROWS, Db)
    sc = torch.tensor([-0.3, 0.7], device=DEV)   # [-2] bytes, [-1] tokens
    gouts = [rnd(B, T, D) for _ in range(3)]
    toks = torch.from_numpy(gi.fineweb_like_tokens(12345, B, T, vocab=VOCAB)).to(DEV)
    ids = torch.randint(0, BYTE_ROWS, (B, T * bpt), generator=g, device=DEV, dtype=torch.int64)
    e = 2 if dtype == torch.bfloat16 else 4
    rec = {"record": "split_x0", "rows": B, "tokens_per_row": T, "tokens": N, "model_dim": D, "byte_dim": Db, "bpt": bpt, "vocab": VOCAB,
           "dtype": str(dtype).replace("torch.", ""), "reps": reps, "algorithmic_mb_ids_given": round(N * (4 + 8 * bpt + e * D + 3 * e * D) / 1e6, 1)}

    one = lambda et, eb, s: mot.split_x0(toks, et, eb, s[1:2], s[0:1], bpt=bpt, ids=ids)

    def eager(et, eb, s):
        x0t = F.rms_norm(F.embedding(toks, et), (D,), eps=F32_EPS)
        x0b = F.rms_norm(F.embedding(ids.view(B, T, bpt), eb), (Db,), eps=F32_EPS).view(B, T, D)
        return x0t, x0b, x0t * s[-1] + x0b * s[-2]

    def composed(et, eb, s):
        x = mot.embed_mix(toks, et, eb, mode="sum", bpt=bpt, ids_a=ids, norm_tok=True, norm_byte=True, norm_out=False, eps=F32_EPS,
                          scale_tok=s[1:2], scale_byte=s[0:1])
        x0t = mot.embed_mix(toks, et, None, mode="noop", norm_tok=True, eps=F32_EPS)
        x0b = F.rms_norm(F.embedding(ids.view(B, T, bpt), eb), (Db,), eps=F32_EPS).view(B, T, D)
        return x0t, x0b, x

    outs3 = [torch.empty(B, T, D, dtype=dtype, device=DEV) for _ in range(3)]

    def fill():
        for o in outs3:
            o.fill_(1.0)

    leaves = [Et.clone().requires_grad_(True), Eb.clone().requires_grad_(True), sc.clone().requires_grad_(True)]

    def fwd_bwd(run):
        def f():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(list(run(*leaves)), gouts)
        return f

    with torch.no_grad():
        a, b = one(Et, Eb, sc), composed(Et, Eb, sc)
        rec["fwd_max_diff_vs_b"] = max(float((p.float() - q.float()).abs().max()) for p, q in zip(a, b))
        del a, b
    fwd = {"one_fwd": lambda: one(Et, Eb, sc), "a_eager_fwd": lambda: eager(Et, Eb, sc), "b_composed_fwd": lambda: composed(Et, Eb, sc), "c_fill_fwd": fill}
    both = {"one_fwd_bwd": fwd_bwd(one), "a_eager_fwd_bwd": fwd_bwd(eager), "b_composed_fwd_bwd": fwd_bwd(composed)}
    with torch.no_grad():
        times = timed_alternating(fwd, reps)
    times.update(timed_alternating(both, reps))
    for k, (med, lo, hi) in times.items():
        rec[k + "_ms"], rec[k + "_min_max_ms"] = med, [lo, hi]
    rec["fwd_faster_than_b"] = times["one_fwd"][2] < times["b_composed_fwd"][1]
    rec["fwd_bwd_faster_than_b"] = times["one_fwd_bwd"][2] < times["b_composed_fwd_bwd"][1]
    rec["fill_over_fwd"] = round(times["c_fill_fwd"][0] / times["one_fwd"][0], 3)
    rec["ratio_fwd_b_over_one"] = round(times["b_composed_fwd"][0] / times["one_fwd"][0], 3)
    rec["ratio_fwd_bwd_b_over_one"] = round(times["b_composed_fwd_bwd"][0] / times["one_fwd_bwd"][0], 3)
    rec["ratio_fwd_bwd_a_over_one"] = round(times["a_eager_fwd_bwd"][0] / times["one_fwd_bwd"][0], 3)
    for k, f in both.items():
        rec[k.replace("_fwd_bwd", "") + "_peak_extra_mb"] = peak_extra_mb(f)
    d = mot._capi.MotSplitX0Desc()   # the shape only: what the size query looks at
    d.struct_size, d.dtype = ctypes.sizeof(d), mot._capi.dtype_code(dtype)
    d.n_rows, d.tokens_per_row, d.bpt, d.id_source = B, T, bpt, mot._capi.IDS_GIVEN
    d.tok_rows, d.byte_rows, d.model_dim, d.byte_dim = VOCAB, BYTE_ROWS, D, Db
    rec["fwd_workspace_mb"] = round(mot._capi.lib.mot_splitx_workspace_bytes(ctypes.byref(d), 0) / 2 ** 20, 3)
    rec["bwd_workspace_mb"] = round(mot._capi.lib.mot_splitx_workspace_bytes(ctypes.byref(d), 1) / 2 ** 20, 1)
    mot.check_status()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the run's own step in bf16 only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    shapes = [(1, 65536, 1024, 64, 16, torch.bfloat16)]
    if not args.quick:
        shapes += [(1, 65536, 1024, 64, 16, torch.float32), (256, 2048, 768, 48, 16, torch.bfloat16), (256, 2048, 768, 48, 16, torch.float32)]
    lines = []
    for shape in shapes:
        lines.append(json.dumps(case(*shape, args.reps)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
        mot.functional.release_workspaces()
        if args.out:   # after every shape: a later shape that runs out of time loses nothing
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
