"""Writes tests/golden/plain_head.npz: the reference's own plain cross-entropy loss run on CPU with autograd, for the seeded inputs
of tests/plain_head_ref.case_inputs (B 4, T 16, D 32, V 128 and 256).

"math":  slice_logits_and_targets is AST-extracted from mathblations/data.py of a reference checkout at generation time and run
         on logits = lm_head(F.rms_norm(x)).float() (model.py:337-338) with the case's y_indices, then F.cross_entropy, the argmax
         accuracy over the sliced rows and the number of sequences whose window is all right (main.py:166-187).
"infer": nn.Linear on the hidden states, the shift and torch.nn.CrossEntropyLoss() of inference/inference.py:349-359 on labels that
         hold -100 entries.
Nothing of the reference is stored; the generator only checks that the files still hold the calls it follows.  Each case runs in
float64 and in float32.  Stored per case: loss, dx and dW of the float64 run, loss and the float32 run's own error against float64
(relative to the largest float64 element) for loss, dx and dW, the accuracy figures of "math", and the torch version.

    python tools/gen_golden_plain_head.py /path/to/mixture-of-tokenizers
"""
from __future__ import annotations

import ast
import sys
import types
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))
import plain_head_ref as pr  # noqa: E402

FOLLOWED = {   # file -> names it must still use where the generator follows it
    "mathblations/main.py": ("slice_logits_and_targets(", "F.cross_entropy(", ".argmax(dim=-1)", "torch.all("),
    "mathblations/model.py": ("F.rms_norm(", "self.lm_head(x).float()"),
    "inference/inference.py": ("CrossEntropyLoss()", "self.model.lm_head(hidden_states)"),
}


def load_slice(ref: Path):
    for rel, names in FOLLOWED.items():
        txt = (ref / rel).read_text()
        for n in names:
            if n not in txt:
                raise SystemExit(f"{rel} no longer holds {n}")
    src = (ref / "mathblations" / "data.py").read_text()
    picked = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "slice_logits_and_targets"]
    if not picked:
        raise SystemExit("slice_logits_and_targets not found in mathblations/data.py")
    mod = types.ModuleType("ref_mathblations_data")
    mod.__dict__.update({"torch": torch})
    exec(compile(ast.Module(body=picked, type_ignores=[]), "data.py", "exec"), mod.__dict__)
    return mod.slice_logits_and_targets


def run_math(slice_fn, vocab, dtype):
    x, w, y, idx = pr.case_inputs("math", vocab)
    xd = x.to(dtype).clone().requires_grad_(True)
    lm_head = nn.Linear(pr.DIM, vocab, bias=False).to(dtype)
    with torch.no_grad():
        lm_head.weight.copy_(w)
    h = F.rms_norm(xd, (xd.size(-1),))
    logits = lm_head(h)
    logits = logits if dtype == torch.float64 else logits.float()
    token_logits, token_targets = slice_fn(logits, idx, y, None, None)
    loss = F.cross_entropy(token_logits, token_targets)
    loss.backward()
    acc_rows = int((token_logits.argmax(dim=-1) == token_targets).sum())
    full = sum(int(torch.all(logits[i, s:e].argmax(dim=-1) == y[i, s:e])) for i, (s, e) in enumerate(idx.tolist()))
    return loss.detach(), xd.grad, lm_head.weight.grad, (token_targets.numel(), acc_rows, full)


def run_infer(vocab, dtype):
    hidden, w, labels, _ = pr.case_inputs("infer", vocab)
    hd = hidden.to(dtype).clone().requires_grad_(True)
    lm_head = nn.Linear(pr.DIM, vocab, bias=False).to(dtype)
    with torch.no_grad():
        lm_head.weight.copy_(w)
    logits = lm_head(hd)
    shift_logits = logits[..., :-1, :].contiguous()
    shift_labels = labels[..., 1:].contiguous()
    loss = nn.CrossEntropyLoss()(shift_logits.view(-1, shift_logits.size(-1)), shift_labels.view(-1))
    loss.backward()
    return loss.detach(), hd.grad, lm_head.weight.grad, None


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(b.double().abs().max().item(), 1e-300))


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    slice_fn = load_slice(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for kind in pr.KINDS:
        for vocab in pr.VOCABS:
            run = (lambda dt: run_math(slice_fn, vocab, dt)) if kind == "math" else (lambda dt: run_infer(vocab, dt))
            l64, dx64, dw64, acc = run(torch.float64)
            l32, dx32, dw32, acc32 = run(torch.float32)
            assert acc == acc32, "the float32 run predicts other classes: choose inputs with wider margins"
            k = lambda dt, what: pr.case_key(kind, vocab, dt, what)
            out[k("f64", "loss")] = np.array(l64.item(), dtype=np.float64)
            out[k("f64", "dx")] = dx64.numpy()
            out[k("f64", "dW")] = dw64.numpy()
            out[k("f32", "loss")] = np.array(l32.item(), dtype=np.float32)
            out[k("f32", "err")] = np.array([rel(l32, l64), rel(dx32, dx64), rel(dw32, dw64)])
            if acc is not None:
                out[k("f64", "counts")] = np.array(acc, dtype=np.int64)   # scored rows, right rows, sequences all right
    dst = REPO / "tests" / "golden" / "plain_head.npz"
    np.savez_compressed(dst, **out)
    print(f"wrote {dst} ({dst.stat().st_size} bytes, {len(out)} arrays)")
    for k_, v in out.items():
        if k_.endswith("err") or k_.endswith("counts"):
            print(k_, v)


if __name__ == "__main__":
    main()
