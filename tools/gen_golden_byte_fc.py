"""Writes tests/golden/byte_fc.npz: the reference's own linear-on-bytes mixin (modded-nanogpt/runs/71051_mot-in_toks-valemb.py: norm
:130-131, mixin_bytes :225-229, fed as at the call site :312-314) run on CPU with autograd, in float64, float32 and bfloat16, for the
seeded cases of tests/byte_fc_ref.CASES.

`norm` and `mixin_bytes` are AST-extracted from a reference checkout at generation time, as tools/gen_golden_pure_concat.py does;
nothing of them is stored.  One edit is made to the extracted syntax tree, none to its arithmetic: the torch.compile decorator is
dropped (eager CPU execution).  The byte embeddings are handed over in per-token byte order (slot k of every token, shape
(bpt, T, byte_dim)), as oracle/gen_golden.py feeds run 71's mixin_bytes (SURVEY section 7, quirk iii).

The byte ids come from the token->byte table and the CPU oracle's pull_from_left (oracle/), and are stored with the tokens.  Stored
per case: tokens, ids_padded, ids_pulled; the float32 and bfloat16 runs' outputs; the float64 run's output and its three gradients;
of the float32 and bfloat16 runs' gradients (and outputs) only their error against the float64 run (largest difference over largest
element).  Float inputs are regenerated from seeds.  The torch version is recorded.

    python tools/gen_golden_byte_fc.py /path/to/mixture-of-tokenizers
"""
from __future__ import annotations

import os

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import ast  # noqa: E402
import sys  # noqa: E402
from pathlib import Path  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import byte_fc_ref as bf  # noqa: E402
import golden_inputs as gi  # noqa: E402
from oracle import oracle as orc  # noqa: E402

NAMES = {"norm", "mixin_bytes"}
RUN = Path("modded-nanogpt") / "runs" / "71051_mot-in_toks-valemb.py"


def load_reference(ref: Path) -> dict:
    src = (ref / RUN).read_text()
    picked = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    missing = NAMES - {n.name for n in picked}
    if missing:
        raise SystemExit(f"not found in the reference: {sorted(missing)}")
    for n in picked:
        n.decorator_list = []
    import torch.nn.functional as F
    from torch import Tensor, nn
    ns = {"torch": torch, "nn": nn, "F": F, "Tensor": Tensor}
    exec(compile(ast.fix_missing_locations(ast.Module(body=picked, type_ignores=[])), str(RUN), "exec"), ns)
    return ns


def run_case(ns, name: str, toks, pulled, dtype):
    Dm, Db, bpt, B, T, Vt, std, seed = bf.CASES[name]
    Et, Eb, W, g = bf.case_tables(name)
    t = lambda a: torch.tensor(a, dtype=torch.float64).to(dtype)
    embed_tokens, embed_bytes = torch.nn.Embedding(Vt, Dm).to(dtype), torch.nn.Embedding(gi.BYTE_VOCAB, Db).to(dtype)
    byte_fc = torch.nn.Parameter(t(W))
    with torch.no_grad():
        embed_tokens.weight.copy_(t(Et))
        embed_bytes.weight.copy_(t(Eb))
    outs = []
    for b in range(B):   # the reference's forward takes one sequence (token_inputs.ndim == 1): row by row
        byte_inputs = torch.tensor(pulled[b]).long().view(T, bpt).t().contiguous()   # (bpt, T): slot k of every token
        x_toks = embed_tokens(torch.tensor(toks[b]).long())[None]
        x_bytes = embed_bytes(byte_inputs).squeeze()
        outs.append(ns["mixin_bytes"](x_toks, x_bytes, byte_fc))
    out = torch.cat(outs, dim=0)
    out.backward(t(g))
    n = lambda a: a.detach().double().numpy()
    return {"out": n(out), "d_tok": n(embed_tokens.weight.grad), "d_byte": n(embed_bytes.weight.grad), "d_byte_fc": n(byte_fc.grad)}


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    ns = load_reference(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for name, (Dm, Db, bpt, B, T, Vt, std, seed) in bf.CASES.items():
        toks, tab = bf.case_tokens(name), bf.case_ttb(name)
        padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
        pulled = orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
        r64, r32, r16 = (run_case(ns, name, toks, pulled, dt) for dt in (torch.float64, torch.float32, torch.bfloat16))
        out[bf.key(name, "tokens")] = toks.astype(np.int32)
        out[bf.key(name, "ids_padded")] = padded.astype(np.int16)
        out[bf.key(name, "ids_pulled")] = pulled.astype(np.int16)
        out[bf.key(name, "f32/out")] = r32["out"].astype(np.float32)
        out[bf.key(name, "bf16/out")] = r16["out"].astype(np.float32)    # bfloat16 values, widened (exact)
        for what in bf.QUANTITIES:
            out[bf.key(name, f"f64/{what}")] = r64[what].astype(np.float64)
            out[bf.key(name, f"f32err/{what}")] = np.array(bf.rel_err(r32[what], r64[what]))
            out[bf.key(name, f"bf16err/{what}")] = np.array(bf.rel_err(r16[what], r64[what]))
            print(f"{name:20s} {what:9s} reference error against float64: float32 {float(out[bf.key(name, f'f32err/{what}')]):.3e}"
                  f"  bfloat16 {float(out[bf.key(name, f'bf16err/{what}')]):.3e}")
    np.savez_compressed(bf.GOLDEN, **out)
    print(f"wrote {bf.GOLDEN} ({bf.GOLDEN.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
