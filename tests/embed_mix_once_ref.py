"""A plain-torch restatement, with autograd, of the three fused front-end modes whose backward has a write-once form
(mot_embed_mix_bwd_once, include/mot.h): per position n of a batch of N

    a   = E_t[tok[n]];              norm_tok:  a = rms_norm(a);        a  *= s_t
    b_k = E_b[ids[n, k]];           norm_byte: b_k = rms_norm(b_k);    b_k *= s_b
    y   = a + cat_k b_k ("sum"),  cat(a, b_0 .. b_{bpt-1}) ("concat"),  a ("noop");      norm_out: x = rms_norm(y)

with rms_norm(v) = v * rsqrt(mean(v^2) + eps) (F.rms_norm).  `run` evaluates it in one dtype on the given (bfloat16-valued) operands and
returns the output and the gradients for an upstream gradient g.  The CPU oracle has no "concat" mode; for "sum" and "noop" the
float64 run is cross-checked against oracle.embed_mix_bwd(dtype=np.float64) by the GPU test.  Nothing here touches a device.
"""
import numpy as np
import torch

F32_EPS = float(np.finfo(np.float32).eps)
BF16_EPS = 2.0 ** -7          # torch.finfo(torch.bfloat16).eps: what F.rms_norm(eps=None) takes on bfloat16 input


def bf16_valued(a: np.ndarray) -> np.ndarray:
    """float64 array whose values are bfloat16 values (round to nearest even)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().double().numpy()


def make_inputs(seed: int, Vt: int, Dt: int, byte_rows: int, Db: int, N: int, Dm: int) -> dict:
    """Tables and the upstream gradient, ~N(0, 1), bfloat16-valued float64."""
    rs = np.random.RandomState(seed)
    inp = {"Et": bf16_valued(rs.standard_normal((Vt, Dt))), "g": bf16_valued(rs.standard_normal((N, Dm)))}
    inp["Eb"] = bf16_valued(rs.standard_normal((byte_rows, Db))) if Db else None
    return inp


def _rms(v, eps):
    return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps)


def run(toks, ids, inp, *, mode, bpt, norm_tok=False, norm_byte=False, norm_out=False, scales=None, dtype=torch.float64, eps=F32_EPS) -> dict:
    """toks (N,) int, ids (N, bpt) int or None, inp from make_inputs, scales (s_t, s_b) or None.  Returns float64 numpy arrays:
    x, d_tok, d_byte, d_scale_tok, d_scale_byte and abs_scale_tok / abs_scale_byte = sum_n |d s contribution of position n|."""
    toks = torch.as_tensor(np.asarray(toks).reshape(-1), dtype=torch.int64)
    N = toks.numel()
    Et = torch.tensor(inp["Et"], dtype=dtype, requires_grad=True)
    g = torch.tensor(inp["g"], dtype=dtype)
    s_t, s_b = scales if scales is not None else (1.0, 1.0)
    # one copy of each scalar per position: the copies' gradients are the positions' contributions to d s
    st = torch.full((N, 1), s_t, dtype=dtype, requires_grad=True)
    sb = torch.full((N, 1, 1), s_b, dtype=dtype, requires_grad=True)
    a = Et[toks]
    if norm_tok:
        a = _rms(a, eps)
    a = a * st
    Eb = None
    if mode != "noop":
        Eb = torch.tensor(inp["Eb"], dtype=dtype, requires_grad=True)
        b = Eb[torch.as_tensor(np.asarray(ids).reshape(N, bpt), dtype=torch.int64)]
        if norm_byte:
            b = _rms(b, eps)
        b = (b * sb).reshape(N, -1)
        y = a + b if mode == "sum" else torch.cat([a, b], dim=1)
    else:
        y = a
    x = _rms(y, eps) if norm_out else y
    x.backward(g)
    f64 = lambda t: None if t is None else t.detach().double().numpy()
    out = {"x": f64(x), "d_tok": f64(Et.grad), "d_byte": f64(Eb.grad) if Eb is not None else None}
    out["d_scale_tok"], out["abs_scale_tok"] = float(st.grad.double().sum()), float(st.grad.double().abs().sum())
    if Eb is not None:
        out["d_scale_byte"], out["abs_scale_byte"] = float(sb.grad.double().sum()), float(sb.grad.double().abs().sum())
    return out
