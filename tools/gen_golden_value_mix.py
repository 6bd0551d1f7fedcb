"""Writes tests/golden/value_mix.npz: the reference's own mixture-of-tokenizers value embeddings (modded-nanogpt/runs/
9_mot-in_mot-valemb.py: norm :130-131, mixin_bytes :225-235, fed as at the call site :310-313) run on CPU with autograd, in float64,
float32 and bfloat16, for the seeded cases of tests/value_mix_ref.CASES.

`norm` and `mixin_bytes` are AST-extracted from a reference checkout at generation time, as tools/gen_golden_byte_fc.py does;
nothing of them is stored.  Two edits are made to the extracted syntax tree, none to its arithmetic: the torch.compile decorator is
dropped (eager CPU execution), and the constant of the assignment ``bpt = 16`` inside mixin_bytes becomes the case's bytes per token
(the run hard-codes its own 16; the case with bpt 16 runs the function as it stands).  The value tables are indexed as at the call
site: ``value_embed(token_inputs)[None]`` and ``value_embed(byte_inputs).squeeze()[None]`` with byte_inputs in per-token byte order.

The byte ids come from the token->byte table and the CPU oracle's pull_from_left (oracle/), and are stored with the tokens.  Stored
per case: tokens, ids_padded, ids_pulled; per slot the float32 and bfloat16 runs' outputs, the float64 run's output and its three
gradients, and of the float32 and bfloat16 runs' gradients (and outputs) their error against the float64 run (largest difference
over largest element).  Float inputs are regenerated from seeds.  The torch version is recorded.

    python tools/gen_golden_value_mix.py /path/to/mixture-of-tokenizers
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
import golden_inputs as gi  # noqa: E402
import value_mix_ref as vm  # noqa: E402
from oracle import oracle as orc  # noqa: E402

NAMES = {"norm", "mixin_bytes"}
RUN = Path("modded-nanogpt") / "runs" / "9_mot-in_mot-valemb.py"


def load_reference(ref: Path, bpt: int) -> dict:
    src = (ref / RUN).read_text()
    picked = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    missing = NAMES - {n.name for n in picked}
    if missing:
        raise SystemExit(f"not found in the reference: {sorted(missing)}")
    edits = 0
    for n in picked:
        n.decorator_list = []
        for a in ast.walk(n):
            if isinstance(a, ast.Assign) and len(a.targets) == 1 and isinstance(a.targets[0], ast.Name) and a.targets[0].id == "bpt":
                assert isinstance(a.value, ast.Constant) and a.value.value == 16
                a.value = ast.Constant(bpt)
                edits += 1
    if edits != 1:
        raise SystemExit(f"expected one `bpt = 16` in mixin_bytes, found {edits}")
    import torch.nn.functional as F
    from torch import Tensor, nn
    ns = {"torch": torch, "nn": nn, "F": F, "Tensor": Tensor}
    exec(compile(ast.fix_missing_locations(ast.Module(body=picked, type_ignores=[])), str(RUN), "exec"), ns)
    return ns


def run_case(ns, name: str, toks, pulled, dtype):
    Dt, Db, bpt, Do, B, T, S, Vt, std, seed = vm.CASES[name]
    t = lambda a: torch.tensor(a, dtype=torch.float64).to(dtype)
    n = lambda a: a.detach().double().numpy()
    res = []
    for Et, Eb, W, g in vm.case_tables(name):
        value_embed_toks, value_embed_bytes = torch.nn.Embedding(Vt, Dt).to(dtype), torch.nn.Embedding(gi.BYTE_VOCAB, Db).to(dtype)
        weight = torch.nn.Parameter(t(W))
        with torch.no_grad():
            value_embed_toks.weight.copy_(t(Et))
            value_embed_bytes.weight.copy_(t(Eb))
        outs = []
        for b in range(B):   # the reference's forward takes one sequence (token_inputs.ndim == 1): row by row
            token_inputs, byte_inputs = torch.tensor(toks[b]).long(), torch.tensor(pulled[b]).long()   # (T,), (T*bpt,) per-token byte order
            vet = value_embed_toks(token_inputs)[None]
            veb = value_embed_bytes(byte_inputs).squeeze()[None]
            outs.append(ns["mixin_bytes"](vet, veb, weight))
        out = torch.cat(outs, dim=0)
        out.backward(t(g))
        res.append({"out": n(out), "d_tok": n(value_embed_toks.weight.grad), "d_byte": n(value_embed_bytes.weight.grad), "d_weight": n(weight.grad)})
    return res


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    out = {"torch_version": np.array(torch.__version__)}
    for name, (Dt, Db, bpt, Do, B, T, S, Vt, std, seed) in vm.CASES.items():
        ns = load_reference(ref, bpt)
        toks, tab = vm.case_tokens(name), vm.case_ttb(name)
        padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
        pulled = orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
        r64, r32, r16 = (run_case(ns, name, toks, pulled, dt) for dt in (torch.float64, torch.float32, torch.bfloat16))
        out[vm.key(name, "tokens")] = toks.astype(np.int32)
        out[vm.key(name, "ids_padded")] = padded.astype(np.int16)
        out[vm.key(name, "ids_pulled")] = pulled.astype(np.int16)
        for j in range(S):
            out[vm.key(name, f"{j}/f32/out")] = r32[j]["out"].astype(np.float32)
            out[vm.key(name, f"{j}/bf16/out")] = r16[j]["out"].astype(np.float32)    # bfloat16 values, widened (exact)
            for what in vm.QUANTITIES:
                out[vm.key(name, f"{j}/f64/{what}")] = r64[j][what].astype(np.float64)
                out[vm.key(name, f"{j}/f32err/{what}")] = np.array(vm.rel_err(r32[j][what], r64[j][what]))
                out[vm.key(name, f"{j}/bf16err/{what}")] = np.array(vm.rel_err(r16[j][what], r64[j][what]))
                print(f"{name:20s} slot {j} {what:9s} reference error against float64: float32 {float(out[vm.key(name, f'{j}/f32err/{what}')]):.3e}"
                      f"  bfloat16 {float(out[vm.key(name, f'{j}/bf16err/{what}')]):.3e}")
    np.savez_compressed(vm.GOLDEN, **out)
    print(f"wrote {vm.GOLDEN} ({vm.GOLDEN.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
