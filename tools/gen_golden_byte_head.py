"""Writes tests/golden/byte_head.npz: the reference's own byte output head (scaled-pre-train/train_gpt.py:483-542, 618-623) run on
CPU with autograd, for the seeded inputs of tests/byte_head_ref.case_inputs.

The classes are AST-extracted from a reference checkout at generation time (norm, CastedLinear, ByteSelfAttn, ByteMixoutCopy /
Split / Noop, ByteMixout, next_multiple_of_n, ByteHyperparameters, ModelDims), as oracle/gen_golden.py does; nothing of it is
stored.  Cases: copy and split, n_layer_out 0, 1, 2, in float64, float32 and eager bfloat16 (x in bf16, CastedLinear casting its
fp32 weight).  Stored: loss, dx and dW of every case (float64 cases in float64, the others in float32), the byte states of the
float64 cases, and the torch version.

    python tools/gen_golden_byte_head.py /path/to/mixture-of-tokenizers
"""
from __future__ import annotations

import ast
import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))
import byte_head_ref as br  # noqa: E402

NAMES = {"norm", "CastedLinear", "ByteSelfAttn", "ByteMixoutCopy", "ByteMixoutSplit", "ByteMixoutNoop", "ByteMixout",
         "next_multiple_of_n", "ByteHyperparameters", "ModelDims"}


def load_reference(ref: Path) -> dict:
    src = (ref / "scaled-pre-train" / "train_gpt.py").read_text()
    picked = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in NAMES]
    missing = NAMES - {n.name for n in picked}
    if missing:
        raise SystemExit(f"not found in the reference: {sorted(missing)}")
    import dataclasses
    import typing

    import einops
    import torch.nn.functional as F
    from torch import Tensor, nn
    ns = {"torch": torch, "nn": nn, "F": F, "Tensor": Tensor, "einops": einops, "dataclass": dataclasses.dataclass,
          "Literal": typing.Literal, "__name__": "ref_train_gpt"}
    import types
    mod = types.ModuleType("ref_train_gpt")
    mod.__dict__.update(ns)
    sys.modules["ref_train_gpt"] = mod   # dataclasses look their class's module up
    ns = mod.__dict__
    exec(compile(ast.Module(body=picked, type_ignores=[]), "train_gpt.py", "exec"), ns)
    return ns


def run_case(ns, method, n_layer_out, dtype):
    x, w, t = br.case_inputs(method, n_layer_out)
    D = x.shape[1]
    bp = ns["ByteHyperparameters"](bytes_per_token=br.BPT, byte_mixout_method=method, n_layer_out=n_layer_out)
    dims = ns["ModelDims"](model_dim=D, byte_dim=D, token_dim=D)
    mixout = ns["ByteMixout"](dims, br.N_TOKENS, bp)
    K = D if method == "copy" else D // br.BPT
    V = ns["next_multiple_of_n"](bp.vocab_size, n=128)
    assert V == br.VOCAB
    lm_head = ns["CastedLinear"](K, V)
    wdt = torch.float64 if dtype == torch.float64 else torch.float32
    lm_head = lm_head.to(wdt)
    with torch.no_grad():
        lm_head.weight.copy_(w.to(wdt))
    xd = x.to(dtype)[None].clone().requires_grad_(True)   # (1, T, D), as GPT.forward sees it
    h = mixout(xd)
    logits = lm_head(ns["norm"](h))
    logits = 30 * torch.sigmoid((logits.double() if dtype == torch.float64 else logits.float()) / 7.5)
    loss = torch.nn.functional.cross_entropy(logits.view(-1, logits.size(-1)), t.view(-1).long())
    loss.backward()
    return h.detach()[0], loss.detach(), xd.grad[0], lm_head.weight.grad


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    ns = load_reference(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for method in ("copy", "split"):
        for L in br.LAYERS:
            for name, dt in (("f64", torch.float64), ("f32", torch.float32), ("bf16", torch.bfloat16)):
                h, loss, dx, dW = run_case(ns, method, L, dt)
                st = np.float64 if dt == torch.float64 else np.float32
                k = lambda what: br.case_key(method, L, name, what)
                out[k("loss")] = np.array(loss.double().item(), dtype=np.float64)
                out[k("dx")] = dx.double().numpy().astype(st)
                out[k("dW")] = dW.double().numpy().astype(st)
                if dt == torch.float64:
                    out[k("states")] = h.numpy()
    dst = REPO / "tests" / "golden" / "byte_head.npz"
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({dst.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
