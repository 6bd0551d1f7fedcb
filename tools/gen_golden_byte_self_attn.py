"""Writes tests/golden/byte_self_attn.npz: the reference's own ByteSelfAttn (scaled-pre-train/train_gpt.py:382-418 around
CausalSelfAttention, Rotary, norm) run on CPU with autograd, in float64 and float32, for the seeded inputs of
tests/byte_self_attn_ref.case_inputs.

The classes are AST-extracted from a reference checkout at generation time (norm, CastedLinear, Rotary, CausalSelfAttention,
ByteSelfAttn, ByteHyperparameters), as tools/gen_golden_byte_head.py does; nothing of it is stored.  They are executed in a
namespace in which create_block_mask builds its mask on the CPU and flex_attention is torch's own eager one (it materialises the
scores: fine at fixture size), with TORCHDYNAMO_DISABLE=1.  c_proj, which the reference zero-initialises, is filled from the
seeded inputs.  Stored per case: out, dx and the gradients of qkv_w, c_proj.weight and lambdas of the float64 run, in float64 (the weight gradients of
the two-head case in float32); of the float32 run the error of every quantity (out, attn = out - x formed in float64, dx, the three
gradients) against the float64 run, as the largest difference over the largest float64 element -- the figure the GPU tests double
for their bar -- not the arrays, so that the fixture stays small; and the torch version.  No committed file may exceed 1 MiB, so
the arrays are packed into byte_self_attn.npz and continuation files byte_self_attn.<k>.npz.  Inputs are regenerated from seeds.

    python tools/gen_golden_byte_self_attn.py /path/to/mixture-of-tokenizers
"""
from __future__ import annotations

import os

os.environ.setdefault("TORCHDYNAMO_DISABLE", "1")

import ast  # noqa: E402
import functools  # noqa: E402
import sys  # noqa: E402
import types  # noqa: E402
from pathlib import Path  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests"))
import byte_self_attn_ref as br  # noqa: E402

NAMES = {"norm", "CastedLinear", "Rotary", "CausalSelfAttention", "ByteSelfAttn", "ByteHyperparameters"}


def load_reference(ref: Path) -> dict:
    src = (ref / "scaled-pre-train" / "train_gpt.py").read_text()
    picked = [n for n in ast.parse(src).body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in NAMES]
    missing = NAMES - {n.name for n in picked}
    if missing:
        raise SystemExit(f"not found in the reference: {sorted(missing)}")
    import dataclasses
    import typing

    import torch.nn.functional as F
    from torch import Tensor, nn
    from torch.nn.attention.flex_attention import BlockMask, create_block_mask, flex_attention
    mod = types.ModuleType("ref_train_gpt")
    mod.__dict__.update({"torch": torch, "nn": nn, "F": F, "Tensor": Tensor, "dataclass": dataclasses.dataclass, "Literal": typing.Literal,
                         "BlockMask": BlockMask, "create_block_mask": functools.partial(create_block_mask, device="cpu"),
                         "flex_attention": flex_attention, "__name__": "ref_train_gpt"})
    sys.modules["ref_train_gpt"] = mod   # dataclasses look their class's module up
    ns = mod.__dict__
    exec(compile(ast.Module(body=picked, type_ignores=[]), "train_gpt.py", "exec"), ns)
    return ns


def run_case(ns, name: str, dtype):
    (x, qkv_w, proj_w, lambdas, g), kw = br.case_inputs(name)
    D, B, T, bpt, swt, bc = br.CASES[name]
    bp = ns["ByteHyperparameters"](bytes_per_token=bpt, use_byte_self_attn=True, sliding_window_tokens=swt)
    layer = ns["ByteSelfAttn"](D, T, bp, mix_byte_in_tok=bc).to(dtype)
    a = layer.attention
    assert a.num_heads == br.n_heads(D) and tuple(a.qkv_w.shape) == tuple(qkv_w.shape)
    with torch.no_grad():
        a.qkv_w.copy_(qkv_w.to(dtype))
        a.c_proj.weight.copy_(proj_w.to(dtype))
        a.lambdas.copy_(lambdas.to(dtype))
    xd = x.to(dtype).clone().requires_grad_(True)
    out = layer(xd)
    out.backward(g.to(dtype))
    return {"out": out.detach(), "attn": out.detach().double() - x.double(), "dx": xd.grad, "dqkv_w": a.qkv_w.grad,
            "dproj_w": a.c_proj.weight.grad, "dlambdas": a.lambdas.grad}


MAX_FILE = 900 * 1024   # no committed file may exceed 1 MiB: the arrays are packed into byte_self_attn.npz, byte_self_attn.1.npz, ...


def main():
    ref = Path(sys.argv[1] if len(sys.argv) > 1 else "../mixture-of-tokenizers")
    ns = load_reference(ref)
    out = {"torch_version": np.array(torch.__version__)}
    for name in br.CASES:
        r64, r32 = run_case(ns, name, torch.float64), run_case(ns, name, torch.float32)
        for what in br.STORED:
            st = np.float32 if what in ("dqkv_w", "dproj_w") and name in br.F32_WEIGHT_GRADS else np.float64
            out[br.case_key(name, "f64", what)] = r64[what].double().numpy().astype(st)
        for what in br.QUANTITIES:   # the float32 run enters as its error against the float64 run, the figure that sets the GPU bar
            out[br.case_key(name, "f32err", what)] = np.array(br.rel_err(r32[what], r64[what]), dtype=np.float64)
            print(f"{name:18s} {what:9s} float32 reference error {float(out[br.case_key(name, 'f32err', what)]):.3e}")
    gold = REPO / "tests" / "golden"
    for old in [gold / "byte_self_attn.npz", *gold.glob("byte_self_attn.*.npz")]:
        old.unlink(missing_ok=True)
    files, size = [{}], 0
    for k, v in out.items():
        if size and size + v.nbytes > MAX_FILE:
            files.append({})
            size = 0
        files[-1][k] = v
        size += v.nbytes
    for i, arrays in enumerate(files):
        dst = gold / ("byte_self_attn.npz" if i == 0 else f"byte_self_attn.{i}.npz")
        np.savez_compressed(dst, **arrays)
        print(f"wrote {dst} ({dst.stat().st_size} bytes, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
