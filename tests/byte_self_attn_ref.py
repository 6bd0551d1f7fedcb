"""A plain-torch restatement of ByteSelfAttn with use_byte_self_attn (scaled-pre-train/train_gpt.py:382-418 around
CausalSelfAttention 209-240, Rotary 189-206, norm 172-173), run eagerly with autograd in any dtype on any device, the queries
taken in chunks so that production lengths fit.  Like the reference's Rotary it rounds q and k to float32 on their way into the
rotary step whatever the module's dtype, so its float64 run is "float64 with fp32-rounded rotary inputs", exactly as the reference's is.  tests/golden/byte_self_attn.npz
(tools/gen_golden_byte_self_attn.py) holds the reference's own outputs for the seeded cases below; test_byte_self_attn_capi.py
checks this file against them, the GPU tests use it in float64 as the reference and in float32 as the eager path whose error
sets the bar."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

HEAD_DIM = 128
ATTN_SCALE = 0.12

# name -> (D, B, T, bpt, sliding_window_tokens, block_causal)
CASES = {
    "d48_causal": (48, 2, 25, 4, 3, False),         # two batch rows: a window meets a row start that is not the start of the buffer
    "d48_block": (48, 2, 25, 4, 3, True),
    "d48_w128_causal": (48, 1, 24, 16, 8, False),   # the production window of 128 bytes over a row of 384: full and short windows, tile seams
    "d48_w128_block": (48, 1, 24, 16, 8, True),
    "d256_causal": (256, 2, 16, 4, 3, False),       # two heads
}
F32_WEIGHT_GRADS = {"d256_causal"}   # stored in float32 to keep the fixture small
STORED = ("out", "dx", "dqkv_w", "dproj_w", "dlambdas")   # attn = out - x is formed in float64 by whoever compares
QUANTITIES = ("out", "attn", "dx", "dqkv_w", "dproj_w", "dlambdas")


def n_heads(D: int) -> int:
    return max(1, D // HEAD_DIM)


def rotary_tables(max_len: int, dim: int = HEAD_DIM):
    """Rotary.__init__'s buffers (train_gpt.py:190-197), fp32 (max_len, dim / 2)."""
    angular_freq = (1 / 1024) ** torch.linspace(0, 1, steps=dim // 4, dtype=torch.float32)
    angular_freq = torch.cat([angular_freq, angular_freq.new_zeros(dim // 4)])
    t = torch.arange(max_len, dtype=torch.float32)
    theta = torch.einsum("i,j -> ij", t, angular_freq)
    return theta.cos(), theta.sin()


def _rotary(x_BTHD, cos, sin):
    T = x_BTHD.size(-3)
    assert cos.size(0) >= T
    c, s = cos[None, :T, None, :], sin[None, :T, None, :]
    x1, x2 = x_BTHD.to(dtype=torch.float32).chunk(2, dim=-1)
    y1 = x1 * c + x2 * s
    y2 = x1 * (-s) + x2 * c
    return torch.cat((y1, y2), 3).type_as(x_BTHD)


def byte_self_attn(x, qkv_w, proj_w, lambdas, cos, sin, *, bpt: int, window: int, block_causal: bool, chunk: int = 512):
    """x (B, L, D) -> x + c_proj(attention), steps 1-6 of the layer.  cos / sin on x's device, in the dtype the module's buffers have."""
    B, L, D = x.shape
    H = qkv_w.shape[1] // HEAD_DIM
    q, k, v = F.linear(x, qkv_w.flatten(end_dim=1).type_as(x)).view(B, L, 3 * H, HEAD_DIM).chunk(3, dim=-2)
    q, k = F.rms_norm(q, (HEAD_DIM,)), F.rms_norm(k, (HEAD_DIM,))
    q, k = _rotary(q, cos, sin), _rotary(k, cos, sin)
    v = lambdas[0] * v
    ys = []
    for i0 in range(0, L, chunk):
        i1 = min(L, i0 + chunk)
        j0, j1 = max(0, i0 - window + 1), min(L, i1 + (bpt - 1 if block_causal else 0))
        qi = torch.arange(i0, i1, device=x.device)[:, None]
        kj = torch.arange(j0, j1, device=x.device)[None, :]
        allowed = (qi // bpt >= kj // bpt) if block_causal else (qi >= kj)
        allowed = allowed & (qi - kj < window)
        s = torch.einsum("bihd,bjhd->bhij", q[:, i0:i1], k[:, j0:j1]) * ATTN_SCALE
        s = s.masked_fill(~allowed, float("-inf"))
        p = torch.softmax(s, dim=-1)
        ys.append(torch.einsum("bhij,bjhd->bihd", p, v[:, j0:j1]))
    y = torch.cat(ys, dim=1).reshape(B, L, H * HEAD_DIM)
    return x + F.linear(y, proj_w.type_as(y))


def run(x, qkv_w, proj_w, lambdas, grad_out, *, bpt, window, block_causal, dtype=torch.float64, device=None, chunk: int = 512):
    """Eager forward + backward in `dtype` on `device`; returns the QUANTITIES in float64 on that device."""
    dev = torch.device(device) if device is not None else x.device
    leaf = lambda t: t.detach().to(device=dev, dtype=dtype).clone().requires_grad_(True)
    xd, wd, pd, ld = leaf(x), leaf(qkv_w), leaf(proj_w), leaf(lambdas)
    # module.to(dtype) casts the Rotary buffers too: in a float64 module the fp32-rounded q, k meet float64 tables and the products
    # run in float64 ("float64 with fp32-rounded rotary inputs"); in float32 everything is fp32
    cos, sin = (t.to(device=dev, dtype=dtype) for t in rotary_tables(x.shape[1]))
    out = byte_self_attn(xd, wd, pd, ld, cos, sin, bpt=bpt, window=window, block_causal=block_causal, chunk=chunk)
    out.backward(grad_out.detach().to(device=dev, dtype=dtype))
    f = lambda a: a.detach().double()
    return {"out": f(out), "attn": f(out) - f(xd), "dx": f(xd.grad), "dqkv_w": f(wd.grad), "dproj_w": f(pd.grad), "dlambdas": f(ld.grad)}


def make_inputs(seed: int, D: int, B: int, L: int):
    """x (B, L, D) rms-normalised rows as FlexibleEmbedding hands them over, qkv_w in CausalSelfAttention's init, c_proj FILLED at its
    CastedLinear scale (the reference zero-initialises it: out == x and no gradient reaches qkv_w or lambdas), lambdas off 0.5 and
    unequal, grad_out normal.  All fp32."""
    H = n_heads(D)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, L, D)).astype(np.float32)
    x = x / np.sqrt((x.astype(np.float64) ** 2).mean(-1, keepdims=True)).astype(np.float32)
    bound = (3 ** 0.5) * 0.5 * D ** -0.5
    qkv_w = rng.uniform(-bound, bound, (3, H * HEAD_DIM, D)).astype(np.float32)
    pb = (3 ** 0.5) * 0.5 * (H * HEAD_DIM) ** -0.5
    proj_w = rng.uniform(-pb, pb, (D, H * HEAD_DIM)).astype(np.float32)
    lambdas = np.array([0.6, 0.4], dtype=np.float32)
    g = rng.standard_normal((B, L, D)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (x, qkv_w, proj_w, lambdas, g))


def case_inputs(name: str):
    """Seeded inputs of one fixture case -> (x, qkv_w, proj_w, lambdas, grad_out), dict(bpt, window, block_causal)."""
    D, B, T, bpt, swt, bc = CASES[name]
    seed = 2000 + sorted(CASES).index(name)
    return make_inputs(seed, D, B, T * bpt), dict(bpt=bpt, window=swt * bpt, block_causal=bc)


def case_key(name: str, dtype: str, what: str) -> str:
    return f"{name}_{dtype}_{what}"


def load_golden() -> dict:
    """tests/golden/byte_self_attn.npz and its continuation files byte_self_attn.<k>.npz (no committed file exceeds 1 MiB), merged."""
    from pathlib import Path
    gold = Path(__file__).resolve().parent / "golden"
    out = {}
    for f in [gold / "byte_self_attn.npz"] + sorted(gold.glob("byte_self_attn.*.npz")):
        with np.load(f) as z:
            out.update({k: z[k] for k in z.files})
    return out


def golden_case(gold: dict, name: str, x: torch.Tensor) -> tuple[dict, dict]:
    """(float64 reference quantities incl. attn, f32err) of one case: f32err[what] is the error of the reference's own float32 CPU
    run against its float64 run, as rel_err measures it (recorded at generation time; the float32 arrays themselves are not stored)."""
    ref = {w: torch.from_numpy(np.asarray(gold[case_key(name, "f64", w)], dtype=np.float64)) for w in STORED}
    ref["attn"] = ref["out"] - x.double()
    return ref, {w: float(gold[case_key(name, "f32err", w)]) for w in QUANTITIES}


def rel_err(got, ref) -> float:
    """Largest absolute difference as a fraction of the largest reference element."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    got = torch.as_tensor(got).to(device=ref.device, dtype=torch.float64)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))
