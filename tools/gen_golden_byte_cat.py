"""Writes tests/golden/byte_cat.npz: the reference's own bytes-only front-end and byte value embeddings
(modded-nanogpt/runs/5_bytes-in_bytes-valemb.py: norm, reshape_bytes :225-232, fed as at lines 305 and 314) run on CPU with autograd in
float64, float32 and bfloat16, for the seeded cases of tests/byte_cat_ref.CASES.

`norm` and `reshape_bytes` are AST-extracted from a reference checkout at generation time, as tools/gen_golden_pure_concat.py does;
nothing of them is stored.  Two edits are made to the extracted syntax tree, none to its arithmetic: the torch.compile decorator is
dropped (eager CPU execution), and the literal reshape_bytes assigns to its local `bpt` (16 in run 5) is replaced by the case's
bytes per token, so that the same statements also serve the bpt 8 and 4 cases.  Every table is an nn.Embedding fed the pulled ids;
table j goes through line 314 (norm(reshape_bytes(...))) where the case's norm flag is set and through line 305 (reshape_bytes(...))
where it is not.

The byte ids come from the token->byte table and the CPU oracle's pull_from_left (oracle/), and are stored with the tokens.  Stored
per case: tokens, ids_padded, ids_pulled; per table the float32 and the bfloat16 run's output (bfloat16 as its 16-bit patterns);
the float64 run's output and table gradient; of the float32 and bfloat16 runs' gradients only their error against the float64 run
(largest difference over largest element).  Float inputs are regenerated from seeds.  The torch version is recorded.

    python tools/gen_golden_byte_cat.py /path/to/mixture-of-tokenizers
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
import byte_cat_ref as bc  # noqa: E402
import golden_inputs as gi  # noqa: E402
from oracle import oracle as orc  # noqa: E402

NAMES = {"norm", "reshape_bytes"}
RUN = Path("modded-nanogpt") / "runs" / "5_bytes-in_bytes-valemb.py"


class _BptFromCase(ast.NodeTransformer):
    """`bpt = <literal>` inside reshape_bytes -> `bpt = BPT` (a global of the namespace the function runs in)."""

    def __init__(self):
        self.hits = 0

    def visit_Assign(self, node):
        if len(node.targets) == 1 and isinstance(node.targets[0], ast.Name) and node.targets[0].id == "bpt" and isinstance(node.value, ast.Constant):
            self.hits += 1
            node.value = ast.copy_location(ast.Name(id="BPT", ctx=ast.Load()), node.value)
        return node


def load_reference(ref: Path) -> dict:
    src = (ref / RUN).read_text()
    picked = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    missing = NAMES - {n.name for n in picked}
    if missing:
        raise SystemExit(f"not found in the reference: {sorted(missing)}")
    tr = _BptFromCase()
    for n in picked:
        n.decorator_list = []
        if n.name == "reshape_bytes":
            tr.visit(n)
    if tr.hits != 1:
        raise SystemExit(f"expected one `bpt = <literal>` in reshape_bytes, found {tr.hits}")
    import torch.nn.functional as F
    from torch import Tensor, nn
    ns = {"torch": torch, "nn": nn, "F": F, "Tensor": Tensor, "BPT": 16}
    exec(compile(ast.fix_missing_locations(ast.Module(body=picked, type_ignores=[])), str(RUN), "exec"), ns)
    return ns


def run_case(ns, name: str, pulled, dtype):
    Db, bpt, B, T, Vt, norm, std, seed = bc.CASES[name]
    tables, gs = bc.case_tables(name)
    t = lambda a: torch.tensor(a, dtype=torch.float64).to(dtype)
    embeds = [torch.nn.Embedding(gi.BYTE_VOCAB, Db).to(dtype) for _ in tables]
    with torch.no_grad():
        for e, a in zip(embeds, tables):
            e.weight.copy_(t(a))
    ns["BPT"] = bpt
    rows = [[] for _ in embeds]
    for b in range(B):   # the reference's forward takes one sequence (token_inputs.ndim == 1, :303): row by row
        byte_inputs = torch.tensor(pulled[b]).long()
        for j, (e, nm) in enumerate(zip(embeds, norm)):
            y = ns["reshape_bytes"](e(byte_inputs).squeeze()[None])          # :305
            rows[j].append(ns["norm"](y) if nm else y)                       # :314
    outs = [torch.cat(r, dim=0) for r in rows]
    torch.autograd.backward(outs, [t(g) for g in gs])
    n = lambda a: a.detach().double().numpy()
    return {"out": [n(o) for o in outs], "d_table": [n(e.weight.grad) for e in embeds]}


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    ns = load_reference(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for name, (Db, bpt, B, T, Vt, norm, std, seed) in bc.CASES.items():
        toks, tab = bc.case_tokens(name), bc.case_ttb(name)
        padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
        pulled = orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
        r64, r32, r16 = (run_case(ns, name, pulled, dt) for dt in (torch.float64, torch.float32, torch.bfloat16))
        out[bc.key(name, "tokens")] = toks.astype(np.int32)
        out[bc.key(name, "ids_padded")] = padded.astype(np.int16)
        out[bc.key(name, "ids_pulled")] = pulled.astype(np.int16)
        for j in range(len(norm)):
            out[bc.key(name, f"f32/out{j}")] = r32["out"][j].astype(np.float32)
            out[bc.key(name, f"bf16/out{j}")] = torch.tensor(r16["out"][j]).bfloat16().view(torch.int16).numpy()   # the 16-bit patterns
            out[bc.key(name, f"f64/out{j}")] = r64["out"][j]
            out[bc.key(name, f"f64/d_table{j}")] = r64["d_table"][j]
            for tag, r in (("f32err", r32), ("bf16err", r16)):
                out[bc.key(name, f"{tag}/d_table{j}")] = np.array(bc.rel_err(r["d_table"][j], r64["d_table"][j]))
            print(f"{name:18s} table {j}: gradient error against float64: float32 {float(out[bc.key(name, f'f32err/d_table{j}')]):.3e}"
                  f"  bfloat16 {float(out[bc.key(name, f'bf16err/d_table{j}')]):.3e}")
    np.savez_compressed(bc.GOLDEN, **out)
    print(f"wrote {bc.GOLDEN} ({bc.GOLDEN.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
