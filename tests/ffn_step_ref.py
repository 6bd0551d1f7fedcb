"""References for the feed-forward of the character mixer's decode step (functional.char_ffn_step / mot_ffn_step).

ffn_step_ref       a float64 restatement of ``h + w2(silu(w1 n) * w3 n)``, ``n = RMSNorm_w(h)`` (inference/inference.py:121-144, 269)
                   in torch, on whatever device its inputs live on.  ``round_bf16=True`` rounds where the bf16 call rounds: n, a = w1 n,
                   silu(a), b = w3 n, silu(a) * b, the output of w2 and the final sum, each through fp32 to bf16 (the call forms every
                   one of them in fp32 first).
reference_module   the project's mirror classes RMSNorm and FeedForward (modules.py, which restate the same lines) in eager torch, with
                   seeded weights: nn.Linear's default init, the norm weight uniform in [0.8, 1.2]."""
import torch
from torch import nn


def ffn_step_ref(h, norm_w, w1, w2, w3, eps=1e-5, round_bf16=False):
    f = torch.float64
    rnd = (lambda t: t.to(torch.float32).to(torch.bfloat16).to(f)) if round_bf16 else (lambda t: t)
    h, norm_w, w1, w2, w3 = (t.detach().to(f) for t in (h, norm_w, w1, w2, w3))
    rs = 1.0 / torch.sqrt((h * h).mean(-1, keepdim=True) + eps)
    n = rnd((h * rs) * norm_w)
    a, b = rnd(n @ w1.T), rnd(n @ w3.T)
    g = rnd(rnd(a / (1.0 + torch.exp(-a))) * b)
    return rnd(h + rnd(g @ w2.T))


class _Block(nn.Module):
    def __init__(self, args):
        from mixture_of_tokenizers_amd import modules as M
        super().__init__()
        self.ffn_norm = M.RMSNorm(args.dim, eps=args.norm_eps)
        self.feed_forward = M.FeedForward(args)

    def forward(self, h):
        return h + self.feed_forward(self.ffn_norm(h))

    def weights(self):
        ff = self.feed_forward
        return self.ffn_norm.weight, ff.w1.weight, ff.w2.weight, ff.w3.weight


def reference_module(dtype, dim=256, inter=512, seed=0, device=None, eps=1e-5):
    """``h -> h + feed_forward(ffn_norm(h))`` in eager torch, its fp32 weights drawn from `seed` and then cast to `dtype`."""
    from mixture_of_tokenizers_amd import modules as M
    gen_state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        m = _Block(M.ModelArgs(version="two_residual", dim=dim, intermediate_dim=inter, norm_eps=eps))
        with torch.no_grad():
            m.ffn_norm.weight.uniform_(0.8, 1.2)
    finally:
        torch.random.set_rng_state(gen_state)
    return m.to(device=device, dtype=dtype).requires_grad_(False)
