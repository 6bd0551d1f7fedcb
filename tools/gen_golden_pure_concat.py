"""Writes tests/golden/pure_concat.npz: the reference's own pure-concatenation mixin (modded-nanogpt/runs/711_mot-in_toks-valemb.py:
norm, :224-232 mixin_bytes, fed as at the call site :314-316) run on CPU with autograd, in float32 and float64, for the seeded cases
of tests/pure_concat_ref.CASES.

`norm` and `mixin_bytes` are AST-extracted from a reference checkout at generation time, as tools/gen_golden_byte_self_attn.py does;
nothing of them is stored.  Two edits are made to the extracted syntax tree, none to its arithmetic: the torch.compile decorator is
dropped (eager CPU execution), and the literal the function assigns to its local `bpt` (16 in run 711) is replaced by the case's
bytes per token, so that the same statements also serve the bpt 8 and 4 cases.  With two id tensors the byte embeddings handed to
mixin_bytes are embed_bytes(padded) + embed_bytes(pulled), FlexibleEmbedding's padded_and_pulled mode (train_gpt.py:371-379).

The byte ids come from the token->byte table and the CPU oracle's pull_from_left (oracle/), and are stored with the tokens.  Stored
per case: tokens, ids_padded, ids_pulled; the float32 run's output; the float64 run's output and table gradients; of the float32
run's gradients only their error against the float64 run (largest difference over largest element).  Float inputs are regenerated
from seeds.  The torch version is recorded.

    python tools/gen_golden_pure_concat.py /path/to/mixture-of-tokenizers
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
import pure_concat_ref as pc  # noqa: E402
from oracle import oracle as orc  # noqa: E402

NAMES = {"norm", "mixin_bytes"}
RUN = Path("modded-nanogpt") / "runs" / "711_mot-in_toks-valemb.py"


class _BptFromCase(ast.NodeTransformer):
    """`bpt = <literal>` inside mixin_bytes -> `bpt = BPT` (a global of the namespace the function runs in)."""

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
        if n.name == "mixin_bytes":
            tr.visit(n)
    if tr.hits != 1:
        raise SystemExit(f"expected one `bpt = <literal>` in mixin_bytes, found {tr.hits}")
    import torch.nn.functional as F
    from torch import Tensor, nn
    ns = {"torch": torch, "nn": nn, "F": F, "Tensor": Tensor, "BPT": 16}
    exec(compile(ast.fix_missing_locations(ast.Module(body=picked, type_ignores=[])), str(RUN), "exec"), ns)
    return ns


def run_case(ns, name: str, toks, padded, pulled, dtype):
    Dt, Db, bpt, B, T, Vt, dual, seed = pc.CASES[name]
    Et, Eb, g = pc.case_tables(name)
    embed_tokens, embed_bytes = torch.nn.Embedding(Vt, Dt).to(dtype), torch.nn.Embedding(gi.BYTE_VOCAB, Db).to(dtype)
    with torch.no_grad():
        embed_tokens.weight.copy_(torch.tensor(Et, dtype=dtype))
        embed_bytes.weight.copy_(torch.tensor(Eb, dtype=dtype))
    ns["BPT"] = bpt
    outs = []
    for b in range(B):   # the reference's forward takes one sequence (token_inputs.ndim == 1, :303): row by row
        x_toks = embed_tokens(torch.tensor(toks[b]).long())[None]
        x_bytes = embed_bytes(torch.tensor(pulled[b]).long())
        if dual:
            x_bytes = x_bytes + embed_bytes(torch.tensor(padded[b]).long())
        outs.append(ns["mixin_bytes"](x_toks, x_bytes.squeeze()[None]))
    out = torch.cat(outs, dim=0)
    out.backward(torch.tensor(g, dtype=dtype))
    return {"out": out.detach().numpy(), "d_tok": embed_tokens.weight.grad.numpy(), "d_byte": embed_bytes.weight.grad.numpy()}


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    ns = load_reference(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for name, (Dt, Db, bpt, B, T, Vt, dual, seed) in pc.CASES.items():
        toks, tab = pc.case_tokens(name), pc.case_ttb(name)
        padded = orc.tokens_to_bytes(toks, tab.astype(np.float32))
        pulled = orc.pull_from_left(padded, bpt, gi.PAD, gi.EOT)
        r64, r32 = run_case(ns, name, toks, padded, pulled, torch.float64), run_case(ns, name, toks, padded, pulled, torch.float32)
        out[pc.key(name, "tokens")] = toks.astype(np.int32)
        out[pc.key(name, "ids_padded")] = padded.astype(np.int16)
        out[pc.key(name, "ids_pulled")] = pulled.astype(np.int16)
        out[pc.key(name, "f32/out")] = r32["out"].astype(np.float32)
        for what in pc.QUANTITIES:
            out[pc.key(name, f"f64/{what}")] = r64[what].astype(np.float64)
            out[pc.key(name, f"f32err/{what}")] = np.array(pc.rel_err(r32[what], r64[what]))
            print(f"{name:22s} {what:7s} float32 reference error {float(out[pc.key(name, f'f32err/{what}')]):.3e}")
    np.savez_compressed(pc.GOLDEN, **out)
    print(f"wrote {pc.GOLDEN} ({pc.GOLDEN.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
