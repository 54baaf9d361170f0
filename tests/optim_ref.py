"""What the tests of the segmented AdamW and the gradient norm share (csrc/k_optim.hip; include/kasf.h: kasf_adamw_segments, kasf_grad_norm), not a test: the
20,000-float layout of odd segments, two classes, the arrays with canaries, and a numpy fp32 restatement of k_adamw's statements (csrc/k_misc.hip) -- every
operation one IEEE fp32 rounding, as the kernel compiled with -ffp-contract=off does them."""
import numpy as np

F32 = np.float32
N_FLAT, CANARY_FLOATS = 20000, 64
# (begin, numel, class): sizes {1, 2, 3, 4, 5, 16, 17, 4095, 4097, 8193}; begins of all four residues mod 4; gaps of 1..7 elements; [3, 4) and [4, 6) touch and
# share a class (one run), [7, 10) and [10, 14) touch and do not (two runs); [8271, 16464) crosses two chunk boundaries
SEGMENTS = [(3, 1, 0), (4, 2, 0), (7, 3, 1), (10, 4, 0), (21, 5, 0), (29, 16, 1), (47, 17, 1), (69, 4095, 0), (4170, 4097, 1), (8271, 8193, 0)]
# two classes that differ in lr, weight decay and step: (lr, beta1, beta2, eps, weight_decay, step)
CLASSES = [(5e-4, 0.9, 0.999, 1e-8, 0.01, 1), (2e-3, 0.8, 0.99, 1e-6, 0.0, 7)]


def listed_mask(segments=SEGMENTS, n=N_FLAT):
    m = np.zeros(n, bool)
    for b, c, _ in segments:
        assert not m[b:b + c].any()
        m[b:b + c] = True
    return m


def class_of(segments=SEGMENTS, n=N_FLAT):
    k = np.full(n, -1, np.int64)
    for b, c, cls in segments:
        k[b:b + c] = cls
    return k


def bias_corrections(beta1, beta2, step):
    """kasf_adamw_step's: 1 - beta^step in double from the float betas, rounded to float."""
    return F32(1.0 - float(F32(beta1)) ** step), F32(1.0 - float(F32(beta2)) ** step)


def adamw_ref(p, g, m, v, cls, s):
    """k_adamw's statements on fp32 arrays; `s` the fp32 gradient scale.  Returns new (p, m, v)."""
    lr, b1, b2, eps, wd = (F32(x) for x in cls[:5])
    bc1, bc2 = bias_corrections(cls[1], cls[2], cls[5])
    step, isq = lr / bc1, F32(1.0) / np.sqrt(bc2)
    p, g, m, v = (np.asarray(a, F32) for a in (p, g, m, v))
    gr = g * F32(s)
    p = p * (F32(1.0) - lr * wd)
    m = b1 * m + (F32(1.0) - b1) * gr
    v = b2 * v + (F32(1.0) - b2) * gr * gr
    p = p - step * m / (np.sqrt(v) * isq + eps)
    assert p.dtype == m.dtype == v.dtype == F32
    return p, m, v


def expected(arrs, s, segments=SEGMENTS, classes=CLASSES):
    """The four payloads after one update of the listed elements; everything else as it was."""
    p, g, m, v = (a.copy() for a in arrs)
    k = class_of(segments, len(p))
    for c, cls in enumerate(classes):
        sel = k == c
        p[sel], m[sel], v[sel] = adamw_ref(p[sel], g[sel], m[sel], v[sel], cls, s)
    return p, g, m, v


def payloads(seed=0, n=N_FLAT):
    """p, g, m, v of unit scale, v non-negative."""
    r = np.random.default_rng(seed)
    return [r.standard_normal(n).astype(F32), r.standard_normal(n).astype(F32), (0.1 * r.standard_normal(n)).astype(F32),
            (0.01 * r.standard_normal(n) ** 2).astype(F32)]


class Guarded:
    """n floats on a 16-byte boundary with CANARY_FLOATS canary floats (a NaN pattern of its own) on either side."""
    PATTERN = 0x7FC5A5A5

    def __init__(self, data):
        n = len(data)
        self.buf = np.full(n + 2 * CANARY_FLOATS + 4, self.PATTERN, np.uint32).view(F32)
        self.start = CANARY_FLOATS + (-(self.buf.ctypes.data // 4 + CANARY_FLOATS) % 4)
        self.data = self.buf[self.start:self.start + n]
        self.data[:] = data
        assert self.data.ctypes.data % 16 == 0

    def canaries_intact(self):
        w = self.buf.view(np.uint32)
        return bool((w[:self.start] == self.PATTERN).all() and (w[self.start + len(self.data):] == self.PATTERN).all())


def bits(a):
    return np.asarray(a, F32).view(np.uint32)


def norm_ref(g, mask, grad_scale):
    return float(np.sqrt((g[mask].astype(np.float64) ** 2).sum()) * grad_scale)
