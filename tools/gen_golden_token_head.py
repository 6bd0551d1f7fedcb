"""Writes tests/golden/token_head.npz: the reference's own token-level output head run on CPU with autograd, for the seeded inputs
of tests/token_head_ref.case_inputs (V 384, D 64, 40 rows, filled weights).

norm, CastedLinear and next_multiple_of_n are AST-extracted from scaled-pre-train/train_gpt.py of a reference checkout at
generation time, as tools/gen_golden_byte_head.py does, and lines 619-623 of GPT.forward are run on them ("sigmoid30").  The
modded-nanogpt run files train at import, so the three expressions of runs/71_mot-in_toks-valemb.py:331-334 are quoted here, and
checked to be in that file, not imported ("rsqrt15").  Nothing of the reference is stored.  Cases: both softcaps, with the norm
and without it in float64, and with it in the reference's own bfloat16 (x in bf16, the fp32 weight cast by CastedLinear / .bfloat16()).
Stored: loss, dx and dW of every case (float64 cases in float64, bf16 cases in float32) and the torch version.

    python tools/gen_golden_token_head.py /path/to/mixture-of-tokenizers
"""
from __future__ import annotations

import ast
import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))
import token_head_ref as tr  # noqa: E402

NAMES = {"norm", "CastedLinear", "next_multiple_of_n"}
RUN71 = "modded-nanogpt/runs/71_mot-in_toks-valemb.py"
RUN71_LINES = (
    "x = norm(x)",
    "logits: Tensor = F.linear(x.flatten(end_dim=1), self.lm_head_w.bfloat16()).float()",
    "loss = F.cross_entropy(15 * logits * torch.rsqrt(logits.square() + 225), token_targets)",
)


def load_reference(ref: Path) -> dict:
    src = (ref / "scaled-pre-train" / "train_gpt.py").read_text()
    picked = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in NAMES]
    missing = NAMES - {n.name for n in picked}
    if missing:
        raise SystemExit(f"not found in the reference: {sorted(missing)}")
    run71 = (ref / RUN71).read_text()
    for want in RUN71_LINES:
        if want not in run71:
            raise SystemExit(f"{RUN71} no longer holds: {want}")
    from torch import Tensor, nn
    mod = types.ModuleType("ref_train_gpt")
    mod.__dict__.update({"torch": torch, "nn": nn, "F": F, "Tensor": Tensor})
    exec(compile(ast.Module(body=picked, type_ignores=[]), "train_gpt.py", "exec"), mod.__dict__)
    return mod.__dict__


def run_case(ns, kind, norm_in, dtype):
    x, w, t = tr.case_inputs(kind, norm_in)
    V = ns["next_multiple_of_n"](300, n=128)
    assert V == tr.VOCAB == w.shape[0]
    f64 = dtype == torch.float64
    xd = x.to(dtype)[None].clone().requires_grad_(True)   # (1, T, D), as GPT.forward sees it
    h = ns["norm"](xd) if norm_in else xd
    if kind == "sigmoid30":   # train_gpt.py:619-623
        lm_head = ns["CastedLinear"](tr.DIM, V).to(torch.float64 if f64 else torch.float32)
        with torch.no_grad():
            lm_head.weight.copy_(w)
        wp = lm_head.weight
        logits = lm_head(h)
        logits = 30 * torch.sigmoid((logits.double() if f64 else logits.float()) / 7.5)
        loss = F.cross_entropy(logits.view(-1, logits.size(-1)), t.view(-1).long())
    else:                     # runs/71_*.py:331-334
        wp = w.to(torch.float64 if f64 else torch.float32).clone().requires_grad_(True)
        wc = wp if f64 else wp.bfloat16()
        logits = F.linear(h.flatten(end_dim=1), wc)
        logits = logits if f64 else logits.float()
        loss = F.cross_entropy(15 * logits * torch.rsqrt(logits.square() + 225), t)
    loss.backward()
    return loss.detach(), xd.grad[0], wp.grad


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    ns = load_reference(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for kind in tr.SOFTCAPS:
        for norm_in in (True, False):
            for name, dt in (("f64", torch.float64), ("bf16", torch.bfloat16)):
                if name == "bf16" and not norm_in:   # the reference always norms: it has no bf16 run without, and the file stays under 1 MiB
                    continue
                loss, dx, dW = run_case(ns, kind, norm_in, dt)
                st = np.float64 if dt == torch.float64 else np.float32
                k = lambda what: tr.case_key(kind, norm_in, name, what)
                out[k("loss")] = np.array(loss.double().item(), dtype=np.float64)
                out[k("dx")] = dx.double().numpy().astype(st)
                out[k("dW")] = dW.double().numpy().astype(st)
    dst = REPO / "tests" / "golden" / "token_head.npz"
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({dst.stat().st_size} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
