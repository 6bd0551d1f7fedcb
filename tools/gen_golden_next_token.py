#!/usr/bin/env python3
"""Writes tests/golden/next_token.npz: what the reference's generation step computes on seeded logits.

The reference's inference/inference.py is PARSED, never imported: the statements of generate()'s loop body from
`next_token_logits = ...` through `probs = torch.softmax(...)` are compiled from its syntax tree and executed here on the fixture's
logits, over (temperature, top_k, top_p) in {1.0, 0.7} x {0, 1, 50, 256} x {1.0, 0.9, 0.5}, in float32 and in float64.  Stored: the
float32 logits (B 3, V 256, no two equal in a row), the configurations, the float64 run's probs and the float32 run's own error
against it.  None of the reference's text is stored.

    python tools/gen_golden_next_token.py --reference /path/to/reference [--out tests/golden/next_token.npz]
"""
import argparse
import ast
import itertools
import types
from pathlib import Path

import numpy as np
import torch

B, V, SEED = 3, 256, 20241
TEMPERATURES, TOP_KS, TOP_PS = (1.0, 0.7), (0, 1, 50, 256), (1.0, 0.9, 0.5)


def loop_statements(source: str):
    """generate()'s loop statements from the assignment of next_token_logits through the assignment of probs, as one code object."""
    tree = ast.parse(source)
    gen = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "generate")
    loop = next(n for n in gen.body if isinstance(n, ast.For))

    def assigns(stmt, name):
        return isinstance(stmt, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in stmt.targets)

    first = next(i for i, s in enumerate(loop.body) if assigns(s, "next_token_logits"))
    last = next(i for i, s in enumerate(loop.body) if assigns(s, "probs"))
    module = ast.Module(body=loop.body[first:last + 1], type_ignores=[])
    return compile(ast.fix_missing_locations(module), "<reference generation step>", "exec")


def run(code, logits, temperature, top_k, top_p):
    scope = {"torch": torch, "outputs": types.SimpleNamespace(logits=logits[:, None, :].clone()), "temperature": temperature, "top_k": top_k,
             "top_p": top_p}
    exec(code, scope)
    return scope["probs"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project")
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "tests" / "golden" / "next_token.npz"))
    a = ap.parse_args()
    code = loop_statements((Path(a.reference) / "inference" / "inference.py").read_text())
    g = torch.Generator().manual_seed(SEED)
    logits = (torch.randn(B, V, generator=g) * 3.0).float()
    assert all(torch.unique(row).numel() == V for row in logits), "equal logits in a row: change the seed"
    configs = list(itertools.product(TEMPERATURES, TOP_KS, TOP_PS))
    probs64, err32 = [], []
    for t, k, p in configs:
        p64 = run(code, logits.double(), t, k, p)
        p32 = run(code, logits, t, k, p)
        assert p64.dtype == torch.float64 and p32.dtype == torch.float32
        probs64.append(p64.numpy())
        err32.append(float((p32.double() - p64).abs().max()))
    np.savez_compressed(a.out, logits=logits.numpy(), configs=np.array(configs, dtype=np.float64), probs=np.stack(probs64),
                        err32=np.array(err32, dtype=np.float64))
    print(f"{a.out}: {len(configs)} configurations, float32 error up to {max(err32):.3e}")


if __name__ == "__main__":
    main()
