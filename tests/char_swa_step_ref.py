"""numpy restatement of the state that mot_char_swa_step keeps on the device (include/mot.h): ring (B, window, c_v) int32, the
characters of source position s in slot s % window, and pos (B,), the tokens of each row seen so far.  step() does what one call
does to the state and returns, per row, the window slice [max(0, t - window + 1), t] read back OUT OF THE RING in source order:
the character matrix to hand to oracle.char_swa (with the tokens of the same positions), whose last row is row t of the full
sequence (rotary cancels and a window never reaches further back)."""
import numpy as np


def case(seed, B, T, c_v, d, H, hd, Vt, Vc):
    """The input recipe of tests/test_gpu_swa.py (copied: existing test files are not imported from)."""
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)
    rs = np.random.RandomState(seed)
    w = lambda *s: rs.standard_normal(s) / np.sqrt(s[-1])
    return dict(toks=rs.randint(0, Vt, (B, T)).astype(np.int32), cid=rs.randint(0, Vc, (B, T, c_v)).astype(np.int64),
                Et=f32(rs.standard_normal((Vt, d))), Ec=f32(rs.standard_normal((Vc, d))),
                wa=f32(1 + 0.1 * rs.standard_normal(d)), wc=f32(1 + 0.1 * rs.standard_normal(d)),
                wq=f32(w(H * hd, d)), wk=f32(w(H * hd, d)), wv=f32(w(H * hd, d)), wo=f32(w(d, H * hd)))


class RingRef:
    def __init__(self, n_rows, window, c_v):
        self.window, self.c_v = int(window), int(c_v)
        self.ring = np.zeros((n_rows, self.window, self.c_v), dtype=np.int32)
        self.pos = np.zeros(n_rows, dtype=np.int64)

    def step(self, chars):
        """chars (B, c_v): the new tokens' character ids.  Returns [(lo, slice (t - lo + 1, c_v))] per row, t = pos before the call."""
        chars = np.asarray(chars)
        out = []
        for b in range(self.ring.shape[0]):
            t = int(self.pos[b])
            self.ring[b, t % self.window] = chars[b]
            lo = max(0, t - self.window + 1)
            out.append((lo, np.stack([self.ring[b, s % self.window] for s in range(lo, t + 1)]).astype(np.int64)))
            self.pos[b] = t + 1
        return out
