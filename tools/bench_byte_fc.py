"""Linear-on-bytes mixin (mot.byte_fc_mix, x = norm(E_tok[tok] + byte_fc . cat_k E_byte[id_k]), modded-nanogpt/runs/71051_*.py:225-229):
the HIP forward and forward + backward against what a caller had before, all in one run on the same tokens:

  (a) eager torch on the device: F.embedding x 2, F.linear, add, F.rms_norm (and autograd for the backward);
  (b) the tree's only route before this mixin: embed_mix(mode="concat_linear") with the weight [I | byte_fc] (twice the contraction, a
      dense gradient into the identity block).

Shapes: run 71051's (one row of 65 536 tokens, model 1024, byte 64, bpt 16) and 256 x 2048 tokens at the headline dims 768 / 48 / 16,
FineWeb-shaped ids (golden_inputs.fineweb_like_tokens, seed 12345: bench.py's generator and seed), GPT-2 vocabulary, fp32 and bf16,
byte ids from the token->byte table.  Times are device events over warmed repetitions (median ms, [min, max]).  Per record also: the
product's FLOPs (2 tokens model_dim K forward; three such products backward in fp32, four in bf16) over the dense MFMA peak of the
dtype, the algorithmic bytes per token e (2 model_dim) + 2 bpt + 4 over the 8 TB/s peak, and the peak device memory of forward +
backward above the resident tensors, for the HIP path and for (a).  One JSON line per record.

    python tools/bench_byte_fc.py [--out FILE] [--reps N] [--quick]
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
PEAK_HBM_TBS = 8.0                                   # MI355X_MICROARCH.md
PEAK_TFLOPS = {"float32": 157.3, "bfloat16": 2516.6}  # dense MFMA peaks, fp32 / bf16
VOCAB, BPT = gi.GPT2_VOCAB, 16
SHAPES = (("run71051", 1, 65536, 1024, 64), ("headline", 256, 2048, 768, 48))   # name, rows, T, model_dim, byte_dim


def timed(f, reps, warm=3):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
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


def put(rec, key, t):
    med, lo, hi = t
    rec[key + "_ms"] = round(med, 4)
    rec[key + "_min_max_ms"] = [round(lo, 4), round(hi, 4)]


def peak_extra(f):
    """peak device memory of one call of f above what is resident before it, in MiB"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def case(name, rows, T, Dm, Db, dtype, reps, tab_np, toks_np):
    e = 2 if dtype == torch.bfloat16 else 4
    K = BPT * Db
    dname = str(dtype).replace("torch.", "")
    g = torch.Generator(device=DEV).manual_seed(12345)
    Et = torch.randn((VOCAB, Dm), generator=g, device=DEV).to(dtype)
    Eb = torch.randn((gi.BYTE_VOCAB, Db), generator=g, device=DEV).to(dtype)
    bound = 3 ** 0.5 * 0.5 / K ** 0.5
    W = ((torch.rand((Dm, K), generator=g, device=DEV) * 2 - 1) * bound).to(dtype)
    Wc = torch.cat([torch.eye(Dm, device=DEV, dtype=dtype), W], dim=1).contiguous()
    toks = torch.from_numpy(toks_np.reshape(-1)[:rows * T].reshape(rows, T)).to(DEV)
    tab = torch.from_numpy(tab_np).to(DEV)
    N = toks.numel()
    gout = torch.randn((rows, T, Dm), generator=g, device=DEV).to(dtype)
    flops = 2.0 * N * Dm * K
    alg = e * 2 * Dm + 2 * BPT + 4
    rec = {"record": "byte_fc", "shape": name, "rows": rows, "T": T, "tokens": N, "dtype": dname, "model_dim": Dm, "byte_dim": Db, "bpt": BPT,
           "reps": reps, "product_gflop_fwd": round(flops / 1e9, 1), "floor_product_fwd_ms": round(flops / (PEAK_TFLOPS[dname] * 1e12) * 1e3, 4),
           "alg_bytes_per_token": alg, "floor_hbm_fwd_ms": round(alg * N / (PEAK_HBM_TBS * 1e12) * 1e3, 4)}
    kw = dict(bpt=BPT, ttb=tab, pull="left")
    eps = float(torch.finfo(torch.float32).eps)
    with torch.no_grad():
        r = mot.byte_fc_mix(toks, Et, Eb, W, return_ids=True, **kw)
        ids, x_ref = r.ids_pulled, r.x
        put(rec, "hip_fwd_ttb", timed(lambda: mot.byte_fc_mix(toks, Et, Eb, W, **kw), reps))
        put(rec, "hip_fwd_given", timed(lambda: mot.byte_fc_mix(toks, Et, Eb, W, bpt=BPT, ids=ids), reps))
        tl, il = toks.long(), ids.reshape(rows, T, BPT)
        eager = lambda Et_, Eb_, W_: F.rms_norm(F.embedding(tl, Et_) + F.linear(F.embedding(il, Eb_).reshape(rows, T, K), W_), (Dm,))
        rec["a_eager_max_abs_diff"] = float((eager(Et, Eb, W).float() - x_ref.float()).abs().max())
        put(rec, "a_eager_fwd", timed(lambda: eager(Et, Eb, W), reps))
        emul = lambda Et_, Eb_, Wc_: mot.embed_mix(toks, Et_, Eb_, mode="concat_linear", bpt=BPT, ttb=tab, pull="left", weight=Wc_, norm_out=True, eps=eps)
        rec["b_emulation_max_abs_diff"] = float((emul(Et, Eb, Wc).float() - x_ref.float()).abs().max())
        put(rec, "b_emulation_fwd", timed(lambda: emul(Et, Eb, Wc), reps))
    del x_ref
    torch.cuda.empty_cache()

    def fwd_bwd(run, leaves):
        def f():
            for t in leaves:
                t.grad = None
            run().backward(gout)
        return f
    Etg, Ebg, Wg, Wcg = (t.clone().requires_grad_(True) for t in (Et, Eb, W, Wc))
    hip = fwd_bwd(lambda: mot.byte_fc_mix(toks, Etg, Ebg, Wg, **kw), [Etg, Ebg, Wg])
    put(rec, "hip_fwd_bwd_ttb", timed(hip, reps))
    rec["hip_fwd_bwd_peak_extra_mib"] = peak_extra(hip)
    mot.functional.release_workspaces()
    torch.cuda.empty_cache()
    a = fwd_bwd(lambda: eager(Etg, Ebg, Wg), [Etg, Ebg, Wg])
    put(rec, "a_eager_fwd_bwd", timed(a, reps))
    rec["a_eager_fwd_bwd_peak_extra_mib"] = peak_extra(a)
    torch.cuda.empty_cache()
    put(rec, "b_emulation_fwd_bwd", timed(fwd_bwd(lambda: emul(Etg, Ebg, Wcg), [Etg, Ebg, Wcg]), reps))
    for k in ("fwd", "fwd_bwd"):
        ours = rec[f"hip_{k}_ttb_ms"]
        rec[f"speedup_{k}_vs_a"] = round(rec[f"a_eager_{k}_ms"] / ours, 2)
        rec[f"speedup_{k}_vs_b"] = round(rec[f"b_emulation_{k}_ms"] / ours, 2)
    rec["hip_fwd_product_floor_frac"] = round(rec["floor_product_fwd_ms"] / rec["hip_fwd_ttb_ms"], 3)
    mot.check_status()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="run 71051's shape only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    tab = gi.widen_left_pad(gi.load_real_ttb8(), BPT)
    toks = gi.fineweb_like_tokens(12345, 256, 2048, vocab=VOCAB)
    lines = []
    for name, rows, T, Dm, Db in (SHAPES[:1] if args.quick else SHAPES):
        for dtype in (torch.float32, torch.bfloat16):
            lines.append(json.dumps(case(name, rows, T, Dm, Db, dtype, args.reps, tab, toks)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
            mot.functional.release_workspaces()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
