"""Bytes-only front-end and byte value embeddings (functional.byte_cat, modded-nanogpt/runs/5_bytes-in_bytes-valemb.py:225-232, 248,
305, 314): the fused HIP forward and forward + backward against what a caller had before, all in one run on the same tokens:

  (a) eager torch: F.embedding per table + reshape + F.rms_norm on the normed one, forward and forward + backward (its backward is
      one embedding_dense_backward per table);
  (b) n_out single-output calls of byte_cat: what sharing the id stream between the outputs buys;
  (c) a fill_ of the same output bytes, in the same session: the forward is a fill, so this is its ceiling on this box.

Shapes: run 5's step, one row of 65 536 tokens, and 256 x 2048 tokens (FineWeb-shaped ids, golden_inputs.fineweb_like_tokens, seed
12345: bench.py's generator and seed); bpt 16, byte_dim 64 (model_dim 1024); four outputs with norm flags (True, False, False,
False) (run 5) and one normed output (runs 4, 6); bf16 and fp32 tables of 458 rows.
Times are device events over warmed repetitions (median ms, with [min, max]).  Algorithmic bytes per token: R = 4 + 2 bpt (ids from
the token->byte table) or 8 bpt (ids given), once for all outputs; W = n_out e model_dim; `hbm_frac` is (R + W) tokens / time
over the 8 TB/s peak.  `bwd_exact_path_fraction` is the share of the backward's non-zero gradient terms that took the exact global
float atomic instead of the fixed-point LDS sums (counted by the kernel in an untimed call).  One JSON line per record.

    python tools/bench_byte_cat.py [--out FILE] [--reps N] [--quick]
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
PEAK_HBM_TBS = 8.0   # MI355X_MICROARCH.md
DB, BPT, VOCAB = 64, 16, gi.GPT2_VOCAB
DM = DB * BPT


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


def alg_bytes(e, n_out, ids):
    return 4 + (2 if ids == "ttb" else 8) * BPT + n_out * e * DM


def put(rec, key, t, n_tok=None, nbytes=None):
    med, lo, hi = t
    rec[key + "_ms"] = round(med, 4)
    rec[key + "_min_max_ms"] = [round(lo, 4), round(hi, 4)]
    if nbytes:
        rec[key + "_hbm_frac"] = round(nbytes * n_tok / (med * 1e-3) / (PEAK_HBM_TBS * 1e12), 4)


def case(rows, T, n_out, dtype, reps, tab_np, toks_np):
    e = 2 if dtype == torch.bfloat16 else 4
    norm = (True,) + (False,) * (n_out - 1)
    g = torch.Generator(device=DEV).manual_seed(12345)
    tables = [torch.randn((gi.BYTE_VOCAB, DB), generator=g, device=DEV).to(dtype) for _ in range(n_out)]
    toks = torch.from_numpy(toks_np.reshape(-1)[:rows * T].reshape(rows, T)).to(DEV)
    tab = torch.from_numpy(tab_np).to(DEV)
    N = toks.numel()
    gouts = [torch.randn((rows, T, DM), generator=g, device=DEV).to(dtype) for _ in range(n_out)]
    rec = {"record": "byte_cat", "rows": rows, "T": T, "tokens": N, "dtype": str(dtype).replace("torch.", ""), "n_out": n_out,
           "byte_dim": DB, "bpt": BPT, "model_dim": DM, "reps": reps,
           "alg_bytes_per_token": {"ttb": alg_bytes(e, n_out, "ttb"), "given": alg_bytes(e, n_out, "given")}}
    kw = dict(bpt=BPT, norm=norm)
    with torch.no_grad():
        outs, _, ids = mot.byte_cat(tables, tokens=toks, ttb=tab, pull="left", return_ids=True, **kw)
        put(rec, "fused_fwd_ttb", timed(lambda: mot.byte_cat(tables, tokens=toks, ttb=tab, pull="left", **kw), reps), N, alg_bytes(e, n_out, "ttb"))
        put(rec, "fused_fwd_given", timed(lambda: mot.byte_cat(tables, ids=ids, **kw), reps), N, alg_bytes(e, n_out, "given"))
        # ---- (a) eager torch
        il = ids.reshape(rows, T, BPT)

        def eager(tabs):
            ys = [F.embedding(il, t).reshape(rows, T, DM) for t in tabs]
            return [F.rms_norm(y, (DM,)) if nm else y for y, nm in zip(ys, norm)]
        rec["eager_max_abs_diff"] = max(float((a.float() - b.float()).abs().max()) for a, b in zip(eager(tables), outs))
        put(rec, "a_eager_fwd", timed(lambda: eager(tables), reps))
        # ---- (b) one call per output
        singles = lambda tabs: [mot.byte_cat([t], bpt=BPT, norm=(nm,), tokens=toks, ttb=tab, pull="left")[0] for t, nm in zip(tabs, norm)]
        put(rec, "b_single_calls_fwd", timed(lambda: singles(tables), reps))
        # ---- (c) a fill of the same output bytes
        bufs = [torch.empty_like(o) for o in outs]

        def fill():
            for b in bufs:
                b.fill_(1.0)
        put(rec, "c_fill", timed(fill, reps), N, n_out * e * DM)
        del bufs, outs
    torch.cuda.empty_cache()

    # ---- forward + backward
    leaves = [t.clone().requires_grad_(True) for t in tables]

    def fwd_bwd(run):
        def f():
            for t in leaves:
                t.grad = None
            torch.autograd.backward(list(run(leaves)), gouts)
        return f
    put(rec, "fused_fwd_bwd_ttb", timed(fwd_bwd(lambda tabs: mot.byte_cat(tabs, tokens=toks, ttb=tab, pull="left", **kw)), reps))
    put(rec, "b_single_calls_fwd_bwd", timed(fwd_bwd(singles), reps))
    put(rec, "a_eager_fwd_bwd", timed(fwd_bwd(eager), reps))
    with torch.no_grad():   # the backward alone, ids given
        det = [t.detach() for t in leaves]
        put(rec, "fused_bwd", timed(lambda: mot.functional.byte_cat_backward(gouts, det, ids=ids, **kw), reps))
        cnt = torch.zeros(2, dtype=torch.int64, device=DEV)   # an untimed call: how many gradient terms left the LDS sums for the exact global path
        mot.functional.byte_cat_backward(gouts, det, ids=ids, counters=cnt, **kw)
        terms, exact = (int(v) for v in cnt.tolist())
        rec["bwd_terms"], rec["bwd_exact_path_terms"], rec["bwd_exact_path_fraction"] = terms, exact, round(exact / max(terms, 1), 8)
    rec["fwd_fraction_of_fill"] = round(rec["c_fill_ms"] / rec["fused_fwd_ttb_ms"], 3)
    rec["speedup_fwd_vs_a"] = round(rec["a_eager_fwd_ms"] / rec["fused_fwd_ttb_ms"], 2)
    rec["speedup_fwd_vs_b"] = round(rec["b_single_calls_fwd_ms"] / rec["fused_fwd_ttb_ms"], 2)
    rec["speedup_fwd_bwd_vs_a"] = round(rec["a_eager_fwd_bwd_ms"] / rec["fused_fwd_bwd_ttb_ms"], 2)
    rec["speedup_fwd_bwd_vs_b"] = round(rec["b_single_calls_fwd_bwd_ms"] / rec["fused_fwd_bwd_ttb_ms"], 2)
    mot.check_status()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="run 5's step only (one row of 65 536 tokens)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    tab = gi.widen_left_pad(gi.load_real_ttb8(), BPT)
    toks = gi.fineweb_like_tokens(12345, 256, 2048, vocab=VOCAB)
    lines = []
    for rows, T in (((1, 65536),) if args.quick else ((1, 65536), (256, 2048))):
        for n_out in (4, 1):
            for dtype in (torch.bfloat16, torch.float32):
                lines.append(json.dumps(case(rows, T, n_out, dtype, args.reps, tab, toks)))
                print(lines[-1], flush=True)
                torch.cuda.empty_cache()
                mot.functional.release_workspaces()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
