"""Writes tests/golden/value_embeds.npz: the reference's own token value embeddings (scaled-pre-train/train_gpt.py: the ModuleList of
line 566 and the list comprehension of line 600) run on CPU with torch's nn.Embedding and autograd in float64, float32 and bfloat16,
for the seeded cases of tests/value_embeds_ref.CASES.

The two statements are AST-extracted from a reference checkout at generation time, as tools/gen_golden_byte_cat.py does; nothing of
them is stored.  They are executed as they stand, in a namespace that supplies the names they read: `self` (an empty nn.Module),
`vocab_size`, `model_dims.model_dim` and `toks_in`.  The tables are then overwritten with the case's seeded values.

Stored per case: the tokens; per table the float64 run's gradient; of the float32 and bfloat16 runs' gradients only their error
against the float64 run (largest difference over largest element).  Float inputs are regenerated from seeds.  The torch version is
recorded.

    python tools/gen_golden_value_embeds.py /path/to/mixture-of-tokenizers
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
from torch import nn  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests"))
import value_embeds_ref as vr  # noqa: E402

SCRIPT = Path("scaled-pre-train") / "train_gpt.py"


def _is_self_value_embeds(node) -> bool:
    return isinstance(node, ast.Attribute) and node.attr == "value_embeds" and isinstance(node.value, ast.Name) and node.value.id == "self"


def load_reference(ref: Path):
    """(code of `self.value_embeds = nn.ModuleList([...])`, code of `ve = [value_embed(toks_in) for value_embed in self.value_embeds]`)"""
    make = look = None
    for node in ast.walk(ast.parse((ref / SCRIPT).read_text())):
        if not isinstance(node, ast.Assign) or len(node.targets) != 1:
            continue
        tgt = node.targets[0]
        if _is_self_value_embeds(tgt) and make is None:
            make = node
        elif (isinstance(tgt, ast.Name) and tgt.id == "ve" and isinstance(node.value, ast.ListComp) and look is None
              and _is_self_value_embeds(node.value.generators[0].iter)):
            look = node
    if make is None or look is None:
        raise SystemExit("the value-embedding statements were not found in the reference")
    code = lambda n: compile(ast.fix_missing_locations(ast.Module(body=[n], type_ignores=[])), f"{SCRIPT}:{n.lineno}", "exec")
    return code(make), code(look)


def run_case(stmts, name: str, dtype):
    vocab, dim, shape, n, kind, seed = vr.CASES[name]
    tables, gs = vr.case_inputs(name)
    t = lambda a: torch.tensor(a, dtype=torch.float64).to(dtype)
    ns = {"nn": nn, "torch": torch, "self": nn.Module(), "vocab_size": vocab, "model_dims": SimpleNamespace(model_dim=dim),
          "toks_in": torch.tensor(vr.case_tokens(name)).long()}
    exec(stmts[0], ns)                                   # :566
    embeds = list(ns["self"].value_embeds)[:n]
    assert len(embeds) == n, f"the reference builds {len(embeds)} tables, the case wants {n}"
    for e, a in zip(embeds, tables):
        e.to(dtype)
        with torch.no_grad():
            e.weight.copy_(t(a))
    exec(stmts[1], ns)                                   # :600
    ve = ns["ve"][:n]
    torch.autograd.backward(ve, [t(g) for g in gs])
    return [e.weight.grad.detach().double().numpy() for e in embeds]


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    stmts = load_reference(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for name, (vocab, dim, shape, n, kind, seed) in vr.CASES.items():
        g64, g32, g16 = (run_case(stmts, name, dt) for dt in (torch.float64, torch.float32, torch.bfloat16))
        out[vr.key(name, "tokens")] = vr.case_tokens(name)
        for j in range(n):
            out[vr.key(name, f"f64/d_table{j}")] = g64[j]
            out[vr.key(name, f"f32err/d_table{j}")] = np.array(vr.rel_err(g32[j], g64[j]))
            out[vr.key(name, f"bf16err/d_table{j}")] = np.array(vr.rel_err(g16[j], g64[j]))
            print(f"{name:16s} table {j}: gradient error against float64: float32 {float(out[vr.key(name, f'f32err/d_table{j}')]):.3e}"
                  f"  bfloat16 {float(out[vr.key(name, f'bf16err/d_table{j}')]):.3e}")
    np.savez_compressed(vr.GOLDEN, **out)
    print(f"wrote {vr.GOLDEN} ({vr.GOLDEN.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
