"""Writes tests/golden/split_x0.npz: the reference's own x0t / x0b / x of modded-nanogpt/runs/71081_mot-in_toks-valemb.py (norm
:128-129; GPT.forward :302-304, 315) run on CPU with autograd, in float64, float32 and bfloat16, for the seeded cases of
tests/split_x0_ref.CASES.

`norm` and the four assignment statements of GPT.forward whose targets are x0t, x0b and x (the first top-level assignment to x: the
later ones are the blocks') are AST-extracted from a reference checkout at generation time, as tools/gen_golden_value_embeds.py does;
nothing of them is stored.  They are executed as they stand against a stub `self` that holds torch nn.Embeddings and a `scalars`
parameter (float32 beside bfloat16 embeddings, as in the run; float64 in the float64 run), one sequence at a time (the run's forward
takes token_inputs.ndim == 1), with byte_inputs (bpt, T): slot k of every token, the per-token byte order.

The byte ids come from the token->byte table and the CPU oracle's pull_from_left (oracle/), and are stored with the tokens.  Stored
per case: tokens, ids; the float32 and bfloat16 runs' three outputs; the float64 run's outputs and its four gradients; and of the
float32 and bfloat16 runs' gradients their error against the float64 run (largest difference over largest element).  Float inputs
are regenerated from seeds.  The torch version is recorded.

    python tools/gen_golden_split_x0.py /path/to/mixture-of-tokenizers
"""
from __future__ import annotations

import os

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import ast  # noqa: E402
import sys  # noqa: E402
from pathlib import Path  # noqa: E402
from types import SimpleNamespace  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import golden_inputs as gi  # noqa: E402
import split_x0_ref as sx  # noqa: E402
from oracle import oracle as orc  # noqa: E402

RUN = Path("modded-nanogpt") / "runs" / "71081_mot-in_toks-valemb.py"
TARGETS = ("x0t", "x0b", "x0b", "x")   # the statements' targets, in source order


def load_reference(ref: Path) -> dict:
    tree = ast.parse((ref / RUN).read_text())
    norm = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "norm"]
    gpt = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "GPT"]
    if len(norm) != 1 or len(gpt) != 1:
        raise SystemExit("norm / class GPT not found in the reference")
    fwd = [n for n in gpt[0].body if isinstance(n, ast.FunctionDef) and n.name == "forward"]
    if len(fwd) != 1:
        raise SystemExit("GPT.forward not found in the reference")
    picked, seen_x = [], False
    for st in fwd[0].body:   # top-level statements only: what the loop over the blocks assigns is the trunk's
        if isinstance(st, ast.Assign) and len(st.targets) == 1 and isinstance(st.targets[0], ast.Name):
            name = st.targets[0].id
            if name in ("x0t", "x0b") or (name == "x" and not seen_x):
                picked.append(st)
                seen_x |= name == "x"
    if tuple(st.targets[0].id for st in picked) != TARGETS:
        raise SystemExit(f"expected assignments to {TARGETS}, found {[st.targets[0].id for st in picked]} at lines {[st.lineno for st in picked]}")
    print("extracted", RUN, "lines", [st.lineno for st in picked])
    norm[0].decorator_list = []
    args = ast.arguments(posonlyargs=[], args=[ast.arg("self"), ast.arg("token_inputs"), ast.arg("byte_inputs")], kwonlyargs=[], kw_defaults=[], defaults=[])
    ret = ast.Return(ast.Tuple([ast.Name(n, ast.Load()) for n in ("x0t", "x0b", "x")], ast.Load()))
    fn = ast.FunctionDef(name="streams", args=args, body=[*picked, ret], decorator_list=[], returns=None, type_params=[])
    import torch.nn.functional as F
    from torch import Tensor, nn
    ns = {"torch": torch, "nn": nn, "F": F, "Tensor": Tensor}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[norm[0], fn], type_ignores=[])), str(RUN), "exec"), ns)
    return ns


def run_case(ns, name: str, toks, ids, dtype) -> dict:
    D, Db, bpt, B, T, Vt, std, seed, absent = sx.CASES[name]
    inp = sx.case_inputs(name)
    t = lambda a: torch.tensor(a, dtype=torch.float64).to(dtype)
    n = lambda a: a.detach().double().numpy()
    embed_tokens, embed_bytes = torch.nn.Embedding(Vt, D).to(dtype), torch.nn.Embedding(gi.BYTE_VOCAB, Db).to(dtype)
    with torch.no_grad():
        embed_tokens.weight.copy_(t(inp["tok_table"]))
        embed_bytes.weight.copy_(t(inp["byte_table"]))
    sdt = torch.float64 if dtype == torch.float64 else torch.float32
    scalars = torch.nn.Parameter(torch.tensor([1.25, sx.S_BYTE, sx.S_TOK], dtype=sdt))   # a longer parameter with the two at its end, as in the run
    stub = SimpleNamespace(embed_tokens=embed_tokens, embed_bytes=embed_bytes, scalars=scalars)
    rows = {w: [] for w in sx.OUTS}
    for b in range(B):   # the reference's forward takes one sequence: row by row
        token_inputs = torch.tensor(toks[b]).long()
        byte_inputs = torch.tensor(ids[b]).long().reshape(T, bpt).t().contiguous()   # (bpt, T): slot k of every token
        for w, o in zip(sx.OUTS, ns["streams"](stub, token_inputs, byte_inputs)):
            rows[w].append(o.reshape(1, T, D))
    outs = {w: torch.cat(rows[w], dim=0) for w in sx.OUTS}
    pairs = [(outs[w], t(g)) for w, g in inp["g"].items() if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    res = {w: n(outs[w]) for w in sx.OUTS}
    res.update(d_tok=n(embed_tokens.weight.grad), d_byte=n(embed_bytes.weight.grad), d_scale_tok=n(scalars.grad[-1]), d_scale_byte=n(scalars.grad[-2]))
    assert float(scalars.grad[0]) == 0.0
    return res


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    ns = load_reference(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for name, (D, Db, bpt, B, T, Vt, std, seed, absent) in sx.CASES.items():
        toks, tab = sx.case_tokens(name), sx.case_ttb(name)
        padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
        ids = orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
        r64, r32, r16 = (run_case(ns, name, toks, ids, dt) for dt in (torch.float64, torch.float32, torch.bfloat16))
        out[sx.key(name, "tokens")] = toks.astype(np.int32)
        out[sx.key(name, "ids")] = ids.astype(np.int16)
        for w in sx.OUTS:
            out[sx.key(name, f"f32/{w}")] = r32[w].astype(np.float32)
            out[sx.key(name, f"bf16/{w}")] = r16[w].astype(np.float32)    # bfloat16 values, widened (exact)
        for what in sx.QUANTITIES:
            out[sx.key(name, f"f64/{what}")] = r64[what].astype(np.float64)
        for what in sx.GRADS:
            out[sx.key(name, f"f32err/{what}")] = np.array(sx.rel_err(r32[what], r64[what]))
            out[sx.key(name, f"bf16err/{what}")] = np.array(sx.rel_err(r16[what], r64[what]))
            print(f"{name:20s} {what:13s} reference error against float64: float32 {float(out[sx.key(name, f'f32err/{what}')]):.3e}"
                  f"  bfloat16 {float(out[sx.key(name, f'bf16err/{what}')]):.3e}")
    np.savez_compressed(sx.GOLDEN, **out)
    print(f"wrote {sx.GOLDEN} ({sx.GOLDEN.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
