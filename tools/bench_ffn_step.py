#!/usr/bin/env python3
"""Times the feed-forward of the character mixer's decode step (functional.char_ffn_step, mot_ffn_step) at config-5 dims -- hidden
2048, intermediate 8192 -- for B = 1, 8, 16 in fp32 and bf16, eagerly and as a replayed hipGraph:
  ffn_fused    the fused call;
  ffn_torch    eager torch ``h + feed_forward(ffn_norm(h))`` with the mirror modules: the baseline, what step() runs by default;
  step_fused   the whole front-end step: char_swa_step followed by the fused call (CharMixerFrontEnd.step(fused_ffn=True));
  step_torch   char_swa_step followed by the torch line (fused_ffn=False).
The method is tools/bench_char_swa_step.py's: device events around REPS consecutive calls, per-call time = elapsed / REPS, the
median of 20 warmed repetitions.  Each figure also as a multiple of the bytes floor at 8 TB/s: w1, w2 and w3 read once, 3 x 2048 x
8192 elements = 201 MB in fp32 (25.2 us), 101 MB in bf16 (12.6 us); the whole step adds wq and wo (33.6 / 16.8 MB).  Back-to-back
calls can find the weights in the 256 MiB Infinity Cache, which a decode loop with a trunk between two steps does not.
usage: bench_ffn_step.py [--out FILE]   (one JSON record per line)"""
import json
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tools"))
import mixture_of_tokenizers_amd as mot  # noqa: E402
from mixture_of_tokenizers_amd import modules as M  # noqa: E402
from bench_char_swa_step import CV, D, DEV, H, HBM_BYTES_PER_S, HD, REPS, ROUNDS, VC, VT, WINDOW, captured, median_us  # noqa: E402

INTER = 8192


def main():
    out = open(sys.argv[sys.argv.index("--out") + 1], "w") if "--out" in sys.argv else None
    g = torch.Generator(device=DEV).manual_seed(1)
    r = lambda *s: torch.randn(s, generator=g, device=DEV)
    w = lambda o, i: r(o, i) / i ** 0.5
    base = dict(Et=r(VT, D), Ec=r(VC, D), wq=w(H * HD, D), wk=w(H * HD, D), wv=w(H * HD, D), wo=w(D, H * HD), wa=1 + 0.1 * r(D), wc=1 + 0.1 * r(D),
                lt=torch.ones(1, device=DEV), lc=torch.ones(1, device=DEV))
    tc = torch.randint(0, VC, (VT, CV), generator=g, device=DEV, dtype=torch.int32)
    torch.manual_seed(2)
    args = M.ModelArgs(version="two_residual", n_heads=H, dim=D, intermediate_dim=INTER, head_dim=HD)
    norm32, ff32 = M.RMSNorm(D, eps=args.norm_eps).to(DEV), M.FeedForward(args).to(DEV)
    with torch.no_grad():
        norm32.weight.uniform_(0.8, 1.2)
    for dtype in ("fp32", "bf16"):
        bf = dtype == "bf16"
        p = {k: v.bfloat16() for k, v in base.items()} if bf else base
        norm, ff = (norm32.bfloat16(), ff32.bfloat16()) if bf else (norm32, ff32)   # (fp32 first: .bfloat16() casts the modules in place)
        kw = dict(attn_norm_w=p["wa"], char_norm_w=p["wc"], wq=p["wq"], wk=p["wk"], wv=p["wv"], wo=p["wo"], n_heads=H, head_dim=HD, window=WINDOW,
                  lambda_tok=p["lt"], lambda_char=p["lc"])
        e = 2 if bf else 4
        ffn_floor, step_floor = 3 * D * INTER * e / HBM_BYTES_PER_S * 1e6, (3 * D * INTER + 2 * D * H * HD) * e / HBM_BYTES_PER_S * 1e6
        for B in (1, 8, 16):
            with torch.no_grad():
                toks = torch.randint(0, VT, (B, 64), generator=g, device=DEV)
                cid = tc[toks].long()
                cache, fcache = {}, {}
                mot.functional.char_swa(toks.to(torch.int32).contiguous(), cid.contiguous(), p["Et"], p["Ec"], kv_cache=cache, **kw)   # fills the key / value tables
                state = mot.char_swa_state(cid[:, :-1], window=WINDOW, c_v=CV)
                tok = toks[:, -1].contiguous()
                swa = lambda: mot.char_swa_step(tok, state, p["Et"], p["Ec"], tok_chars=tc, kv_cache=cache, **kw)   # (the state runs on: any position costs the same)
                h = swa()
                fused = lambda x: mot.char_ffn_step(x, norm.weight, ff.w1.weight, ff.w2.weight, ff.w3.weight, norm_eps=norm.eps, cache=fcache)
                torch_line = lambda x: x + ff(norm(x))
                a, b = fused(h), torch_line(h)
                rec = {"what": "char_ffn_step", "dtype": dtype, "B": B, "dim": D, "inter": INTER,
                       "timing": f"device events, median of {ROUNDS} repetitions of {REPS} calls, us per call",
                       "ffn_weights_floor_us": round(ffn_floor, 2), "step_weights_floor_us": round(step_floor, 2),
                       "fused_vs_torch_rel_diff": float((a.float() - b.float()).abs().max() / b.float().abs().max())}
                fns = (("ffn_fused", lambda: fused(h), ffn_floor), ("ffn_torch", lambda: torch_line(h), ffn_floor),
                       ("step_fused", lambda: fused(swa()), step_floor), ("step_torch", lambda: torch_line(swa()), step_floor))
                for name, fn, floor in fns:
                    for mode, f in (("eager", fn), ("graph", captured(fn))):
                        k = f"{name}_{mode}"
                        rec[k + "_us"], rec[k + "_min_us"], rec[k + "_max_us"] = median_us(f)
                        rec[k + "_x_floor"] = round(rec[k + "_us"] / floor, 2)
                mot.check_status()
                for mode in ("eager", "graph"):
                    rec[f"{mode}_ratio_torch_over_fused_ffn"] = round(rec[f"ffn_torch_{mode}_us"] / rec[f"ffn_fused_{mode}_us"], 2)
                    rec[f"{mode}_ratio_torch_over_fused_step"] = round(rec[f"step_torch_{mode}_us"] / rec[f"step_fused_{mode}_us"], 2)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
