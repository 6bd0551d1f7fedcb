"""Pure-concatenation mixin (mode="concat", x = norm(cat(token row, byte rows)), modded-nanogpt/runs/711_*.py:224-232): the fused HIP
forward and forward + backward against what the tree offered before, all in one run on the same tokens:

  (a) the composition: two gather_rows launches + torch.cat + F.rms_norm (forward only: gather_rows records no autograd node; the
      forward + backward figure beside it is the plain-torch composition F.embedding + torch.cat + F.rms_norm);
  (b) the emulation: mode="concat_linear" with an identity weight (a model_dim x model_dim contraction per token for a copy);
  (c) the un-routed fused SUM kernel at D 768 (byte_dim 48) on the same tokens: 6180 B/token of algorithmic traffic in fp32, the
      same as the concat mode at 512 / 32 / 16, half of it writes instead of two thirds.

Shapes: 256 x 2048 tokens with FineWeb-shaped ids (golden_inputs.fineweb_like_tokens, seed 12345: bench.py's generator and seed)
and their first 32 rows, the 65 536-token shard; token_dim 512, byte_dim 32, bpt 16; fp32 and bf16 tables.
Times are device events over warmed repetitions (median ms).  Algorithmic bytes per token: R = 4 + 2 bpt + e tok_dim (token id,
int16 token->byte row, token row), W = e model_dim; `hbm_frac` is (R + W) tokens / time over the 8 TB/s peak.  With the ids given
as int64 the id traffic is 8 bpt instead of 2 bpt and the record says so.  One JSON line per record.

    python tools/bench_pure_concat.py [--out FILE] [--reps N] [--quick]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import golden_inputs as gi  # noqa: E402
import mixture_of_tokenizers_amd as mot  # noqa: E402

DEV = torch.device("cuda", 0)
PEAK_HBM_TBS = 8.0   # MI355X_MICROARCH.md
DT, DB, BPT, VOCAB = 512, 32, 16, gi.GPT2_VOCAB
SUM_D, SUM_DB = 768, 48


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


def alg_bytes(e, tok_dim, model_dim, ids):
    return 4 + (2 if ids == "ttb" else 8) * BPT + e * tok_dim + e * model_dim


def put(rec, key, t, n_tok=None, nbytes=None):
    med, lo, hi = t
    rec[key + "_ms"] = round(med, 4)
    rec[key + "_min_max_ms"] = [round(lo, 4), round(hi, 4)]
    if nbytes:
        rec[key + "_hbm_frac"] = round(nbytes * n_tok / (med * 1e-3) / (PEAK_HBM_TBS * 1e12), 4)


def case(rows, dtype, reps, tab_np, toks_np):
    e = 2 if dtype == torch.bfloat16 else 4
    Dm = DT + BPT * DB
    g = torch.Generator(device=DEV).manual_seed(12345)
    Et = torch.randn((VOCAB, DT), generator=g, device=DEV).to(dtype)
    Eb = torch.randn((gi.BYTE_VOCAB, DB), generator=g, device=DEV).to(dtype)
    Et768 = torch.randn((VOCAB, SUM_D), generator=g, device=DEV).to(dtype)
    Eb48 = torch.randn((gi.BYTE_VOCAB, SUM_DB), generator=g, device=DEV).to(dtype)
    eye = torch.eye(Dm, device=DEV, dtype=dtype)
    toks = torch.from_numpy(toks_np[:rows]).to(DEV)
    tab = torch.from_numpy(tab_np).to(DEV)
    N = toks.numel()
    gout = torch.randn((rows, toks.shape[1], Dm), generator=g, device=DEV).to(dtype)
    rec = {"record": "pure_concat", "rows": rows, "T": int(toks.shape[1]), "tokens": N, "dtype": str(dtype).replace("torch.", ""),
           "tok_dim": DT, "byte_dim": DB, "bpt": BPT, "model_dim": Dm, "reps": reps,
           "alg_bytes_per_token": {"concat_ttb": alg_bytes(e, DT, Dm, "ttb"), "concat_given": alg_bytes(e, DT, Dm, "given"),
                                   "sum768_ttb": alg_bytes(e, SUM_D, SUM_D, "ttb"), "sum768_given": alg_bytes(e, SUM_D, SUM_D, "given")}}
    kw = dict(mode="concat", bpt=BPT, norm_out=True)
    with torch.no_grad():
        r = mot.embed_mix(toks, Et, Eb, ttb=tab, pull="left", return_ids=True, **kw)
        ids = r.ids_pulled
        x_ref = r.x
        # ---- forward: fused, ids from the token->byte table / ids given
        put(rec, "fused_fwd_ttb", timed(lambda: mot.embed_mix(toks, Et, Eb, ttb=tab, pull="left", **kw), reps), N, alg_bytes(e, DT, Dm, "ttb"))
        put(rec, "fused_fwd_given", timed(lambda: mot.embed_mix(toks, Et, Eb, ids_a=ids, **kw), reps), N, alg_bytes(e, DT, Dm, "given"))
        # ---- (a) two gather_rows + cat + rms_norm
        flat_t, flat_b = toks.reshape(-1), ids.reshape(-1)

        def compose():
            a = mot.gather_rows(Et, flat_t)
            b = mot.gather_rows(Eb, flat_b)
            xc = torch.cat([a.reshape(rows, -1, DT), b.reshape(rows, -1, BPT * DB)], dim=-1)
            return F.rms_norm(xc, (Dm,))
        xa = compose()
        rec["composition_max_abs_diff"] = float((xa.float() - x_ref.float()).abs().max())
        put(rec, "a_composition_fwd", timed(compose, reps))
        del xa
        # ---- (b) concat_linear with an identity weight
        lin = lambda: mot.embed_mix(toks, Et, Eb, mode="concat_linear", bpt=BPT, ids_a=ids, weight=eye, norm_out=True)
        rec["identity_linear_max_abs_diff"] = float((lin().float() - x_ref.float()).abs().max())
        put(rec, "b_identity_linear_fwd", timed(lin, reps))
        # ---- (c) the un-routed SUM kernel at D 768 on the same tokens (ids given never route; below 131 072 tokens nothing routes)
        skw = dict(mode="sum", bpt=BPT, norm_out=True)
        put(rec, "c_sum768_fwd_given", timed(lambda: mot.embed_mix(toks, Et768, Eb48, ids_a=ids, **skw), reps), N, alg_bytes(e, SUM_D, SUM_D, "given"))
        if N < 131072 or dtype == torch.bfloat16:
            put(rec, "c_sum768_fwd_ttb", timed(lambda: mot.embed_mix(toks, Et768, Eb48, ttb=tab, pull="left", **skw), reps), N,
                alg_bytes(e, SUM_D, SUM_D, "ttb"))
    torch.cuda.empty_cache()

    # ---- forward + backward
    def fwd_bwd(run, leaves, gr):
        def f():
            for t in leaves:
                t.grad = None
            run().backward(gr)
        return f
    Etg, Ebg = Et.clone().requires_grad_(True), Eb.clone().requires_grad_(True)
    put(rec, "fused_fwd_bwd_ttb", timed(fwd_bwd(lambda: mot.embed_mix(toks, Etg, Ebg, ttb=tab, pull="left", **kw), [Etg, Ebg], gout), reps))
    tl, il = toks.long(), ids.reshape(rows, -1, BPT)
    eager = lambda: F.rms_norm(torch.cat([F.embedding(tl, Etg), F.embedding(il, Ebg).reshape(rows, -1, BPT * DB)], dim=-1), (Dm,))
    put(rec, "a_torch_composition_fwd_bwd", timed(fwd_bwd(eager, [Etg, Ebg], gout), reps))
    torch.cuda.empty_cache()
    put(rec, "b_identity_linear_fwd_bwd", timed(fwd_bwd(lambda: mot.embed_mix(toks, Etg, Ebg, mode="concat_linear", bpt=BPT, ids_a=ids, weight=eye,
                                                                             norm_out=True), [Etg, Ebg], gout), reps))
    torch.cuda.empty_cache()
    E7, E4 = Et768.clone().requires_grad_(True), Eb48.clone().requires_grad_(True)
    g768 = torch.randn((rows, toks.shape[1], SUM_D), generator=g, device=DEV).to(dtype)
    put(rec, "c_sum768_fwd_bwd_given", timed(fwd_bwd(lambda: mot.embed_mix(toks, E7, E4, ids_a=ids, mode="sum", bpt=BPT, norm_out=True), [E7, E4], g768), reps))
    rec["speedup_fwd_vs_a"] = round(rec["a_composition_fwd_ms"] / rec["fused_fwd_ttb_ms"], 2)
    rec["speedup_fwd_vs_b"] = round(rec["b_identity_linear_fwd_ms"] / rec["fused_fwd_ttb_ms"], 2)
    rec["speedup_fwd_bwd_vs_a_torch"] = round(rec["a_torch_composition_fwd_bwd_ms"] / rec["fused_fwd_bwd_ttb_ms"], 2)
    rec["speedup_fwd_bwd_vs_b"] = round(rec["b_identity_linear_fwd_bwd_ms"] / rec["fused_fwd_bwd_ttb_ms"], 2)
    mot.check_status()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="the 65 536-token shard only")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a timing taken elsewhere says nothing"
    tab = gi.widen_left_pad(gi.load_real_ttb8(), BPT)
    toks = gi.fineweb_like_tokens(12345, 256, 2048, vocab=VOCAB)
    lines = []
    for rows in ((32,) if args.quick else (256, 32)):
        for dtype in (torch.float32, torch.bfloat16):
            lines.append(json.dumps(case(rows, dtype, args.reps, tab, toks)))
            print(lines[-1], flush=True)
            torch.cuda.empty_cache()
            mot.functional.release_workspaces()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
