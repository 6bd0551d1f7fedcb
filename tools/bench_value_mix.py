"""Mixture-of-tokenizers value embeddings (functional.value_mix; modded-nanogpt/runs/9_mot-in_mot-valemb.py:310-313, runs 3 and 6):
one forward and one backward call for all slots against what a caller had before, all in one process on the same tensors, the
variants alternated repetition by repetition:

  (a) one embed_mix(mode="concat_linear", norm_out=True) call per slot: its own index pass, autograd node, token order and dense
      fp32 token-table gradient each (code this library had before value_mix: the parent's path, measured in the same process);
  (b) eager torch: F.embedding twice, cat, F.linear, F.rms_norm per slot.

Shapes: the runs' step (65 536 tokens, three slots, 1024 / 64 / 16 -> 1024, vocabulary 50 257, 458 byte rows) in bf16 and fp32, and
the headline batch (524 288 tokens at 768 / 48 / 16 -> 768, bf16).  Token ids FineWeb-shaped (golden_inputs.fineweb_like_tokens,
seed 12345), byte ids uniform over the byte vocabulary.
Times are device events, the median of `--reps` warmed repetitions (with [min, max]); the whole measurement is repeated `--rounds`
times and (a)'s spread is max - min of its medians over the rounds: "not slower than (a)" means the one-call forward + backward
median (its worst round) is at most (a)'s best round plus that spread.  Peak extra memory is torch's peak allocated bytes over one
forward + backward beyond what was allocated before it (workspaces included: they are dropped before each measurement).
One JSON line per record.

    python tools/bench_value_mix.py [--out FILE] [--reps N] [--rounds N] [--quick]
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
VOCAB, BYTE_ROWS, SLOTS = gi.GPT2_VOCAB, gi.BYTE_VOCAB, 3
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
        out[k] = (v[len(v) // 2], v[0], v[-1])
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


def case(N, Dt, Db, bpt, Do, dtype, reps, rounds):
    K = Dt + bpt * Db
    g = torch.Generator(device=DEV).manual_seed(12345)
    rnd = lambda *shape, s=1.0: (s * torch.randn(shape, generator=g, device=DEV)).to(dtype)
    Vt, Vb = [rnd(VOCAB, Dt) for _ in range(SLOTS)], [rnd(BYTE_ROWS, Db) for _ in range(SLOTS)]
    W = [rnd(Do, K, s=0.5 / K ** 0.5) for _ in range(SLOTS)]
    gouts = [rnd(1, N, Do) for _ in range(SLOTS)]
    toks = torch.from_numpy(gi.fineweb_like_tokens(12345, 1, N, vocab=VOCAB)).to(DEV).reshape(1, N)
    ids = torch.randint(0, BYTE_ROWS, (1, N * bpt), generator=g, device=DEV, dtype=torch.int64)
    rec = {"record": "value_mix", "tokens": N, "token_dim": Dt, "byte_dim": Db, "bpt": bpt, "out_dim": Do, "slots": SLOTS, "vocab": VOCAB,
           "dtype": str(dtype).replace("torch.", ""), "reps": reps, "rounds": rounds}

    one = lambda vt, vb, w: mot.value_mix(toks, vt, vb, w, bpt=bpt, ids=ids)
    three = lambda vt, vb, w: [mot.embed_mix(toks, vt[j], vb[j], mode="concat_linear", bpt=bpt, ids_a=ids, weight=w[j], norm_out=True, eps=F32_EPS)
                               for j in range(SLOTS)]

    def eager(vt, vb, w):
        out = []
        for j in range(SLOTS):
            u = torch.cat([F.embedding(toks, vt[j]), F.embedding(ids, vb[j]).view(1, N, bpt * Db)], dim=-1)
            y = F.linear(u, w[j])
            out.append(F.rms_norm(y, (Do,), eps=F32_EPS))
        return out

    leaves = [[t.clone().requires_grad_(True) for t in ts] for ts in (Vt, Vb, W)]

    def fwd_bwd(run):
        def f():
            for ts in leaves:
                for t in ts:
                    t.grad = None
            torch.autograd.backward(list(run(*leaves)), gouts)
        return f

    with torch.no_grad():
        x1, x3 = one(Vt, Vb, W), three(Vt, Vb, W)
        rec["fwd_max_diff_vs_a"] = max(float((a.float() - b.float()).abs().max()) for a, b in zip(x1, x3))
        del x1, x3
    fwd = {"one_fwd": lambda: one(Vt, Vb, W), "a_three_fwd": lambda: three(Vt, Vb, W), "b_eager_fwd": lambda: eager(Vt, Vb, W)}
    both = {"one_fwd_bwd": fwd_bwd(one), "a_three_fwd_bwd": fwd_bwd(three), "b_eager_fwd_bwd": fwd_bwd(eager)}
    meds = {k: [] for k in (*fwd, *both)}
    for _ in range(rounds):
        with torch.no_grad():
            for k, t in timed_alternating(fwd, reps).items():
                meds[k].append(round(t[0], 4))
        for k, t in timed_alternating(both, reps).items():
            meds[k].append(round(t[0], 4))
    for k, v in meds.items():
        rec[k + "_ms"] = sorted(v)[len(v) // 2]
        rec[k + "_round_medians_ms"] = v
    a = meds["a_three_fwd_bwd"]
    rec["a_spread_ms"] = round(max(a) - min(a), 4)
    rec["not_slower_than_a"] = max(meds["one_fwd_bwd"]) <= min(a) + rec["a_spread_ms"]
    rec["ratio_fwd_bwd_a_over_one"] = round(rec["a_three_fwd_bwd_ms"] / rec["one_fwd_bwd_ms"], 3)
    rec["ratio_fwd_a_over_one"] = round(rec["a_three_fwd_ms"] / rec["one_fwd_ms"], 3)
    rec["ratio_fwd_bwd_b_over_one"] = round(rec["b_eager_fwd_bwd_ms"] / rec["one_fwd_bwd_ms"], 3)
    for k, f in both.items():
        rec[k.replace("_fwd_bwd", "") + "_peak_extra_mb"] = peak_extra_mb(f)
    rec["memory_below_a"] = rec["one_peak_extra_mb"] < rec["a_three_peak_extra_mb"]
    d = mot._capi.MotValueMixDesc()   # the shape only: what the size query looks at
    d.struct_size, d.dtype = ctypes.sizeof(d), mot._capi.dtype_code(dtype)
    d.n_rows, d.tokens_per_row, d.bpt, d.id_source = 1, N, bpt, mot._capi.IDS_GIVEN
    d.tok_rows, d.byte_rows, d.token_dim, d.byte_dim, d.out_dim, d.n_slots, d.norm_out = VOCAB, BYTE_ROWS, Dt, Db, Do, SLOTS, 1
    rec["fwd_workspace_mb"] = round(mot._capi.lib.mot_value_mix_workspace_bytes(ctypes.byref(d), 0) / 2 ** 20, 1)
    rec["bwd_workspace_mb"] = round(mot._capi.lib.mot_value_mix_workspace_bytes(ctypes.byref(d), 1) / 2 ** 20, 1)
    mot.check_status()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the 65 536-token step in bf16 only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    shapes = [(65536, 1024, 64, 16, 1024, torch.bfloat16)]
    if not args.quick:
        shapes += [(65536, 1024, 64, 16, 1024, torch.float32), (524288, 768, 48, 16, 768, torch.bfloat16)]
    lines = []
    for shape in shapes:
        lines.append(json.dumps(case(*shape, args.reps, args.rounds)))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
        mot.functional.release_workspaces()
        if args.out:   # after every shape: a later shape that runs out of time loses nothing
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
