"""The piece rounding of the symmetric fused loss kernel (bce_dense_sym_kernel) as a numpy model, and the embeddings
on which tests/test_gpu_loss_range.py runs the kernel itself.

The kernel forms S = Zt Zt^T and the P V products on the matrix pipe from 16-bit pieces of the fp32 operands: two fp16
pieces (22 mantissa bits, fp16's exponent range) or bf16 pieces (fp32's exponent range; three of them for S, two for
P and V).  Only that rounding is modelled: numpy float16 conversions round to nearest even and keep subnormals, rows
carry log2(e) before the split as in the kernel, and everything after the split is fp64.

Two arrangements of the gradient dZt = (G + G^T) Zt / n^2, G = w sigmoid(S) - pw A, w = 1 + (pw - 1) A:
  * ``model(..., centred=False)``: the rounded Zt against the whole of G.  Two fp16 pieces leave
    |v - hi - lo| <= max(2^-22 |v|, 2^-25) -- the second piece is an fp16 subnormal for |v| < 2^-3 --, so every small
    value's relative error 2^-25 / |z| reaches the gradient undamped; the fp16 form then misses the suite's
    gradient bound from an embedding scale of about 3e-4 downwards.  The kernel does NOT compute this.
  * ``model(..., centred=True)``: what the kernel computes.  G = P + 1/2 + E with P = sigmoid(S) - 1/2 and E the edge
    terms; only P V runs on pieces (P split into two pieces as well), 1/2 colsum(Zt) comes from fp64 column sums of
    the fp32 values and E Zt from the fp32 edge walk.  P -> 0 with the logits, so the piece error of small embeddings
    is multiplied by a small P: the form holds its bound at every scale, down to pieces that are all zero."""
import numpy as np

LOG2E = 1.4426950408889634
TOL = 1e-5                      # the suite's bounds (tests/test_gpu_parity.py): loss TOL max(1, |ref|), gradient 5 TOL
GRAD_BOUND = 5 * TOL
F16_MAX = 32768.0               # kF16Max of decoder_bce.hip: the largest |Zt| that stays on the fp16 pieces
SHAPES = [(641, 16), (1100, 7)]  # (n, d): one tile past a 128-row panel multiple / d < 16 and a 256-row panel tail
LADDER = [1.0, 1e-2, 1e-3, 3e-4, 1e-4, 1e-5, 1e-6, 1e-8]
GUARD_IN = [32768.0, -32768.0]
GUARD_OUT = [float(np.nextafter(np.float32(32768.0), np.float32(np.inf))), 40000.0, 65504.0, -65504.0, 65520.0, 1.0e5]


# ----------------------------------------------------------------- inputs
def sym_edges(n, seed=0):
    """random symmetric multigraph, ~5.5 edges per node: (src, dst) with both directions of every pair"""
    rng = np.random.default_rng(1000 + seed)
    e = 11 * n // 4
    a = rng.integers(0, n, e); b = rng.integers(0, n, e)
    return np.concatenate([a, b]).astype(np.int64), np.concatenate([b, a]).astype(np.int64)


def base(n, d):
    return np.random.default_rng(n * 31 + d).standard_normal((n, d)).astype(np.float32)


def given_mask(n, d):
    """an inverted-dropout mask (p = 0.1) as a caller would hand it in"""
    return ((np.random.default_rng(n + 7 * d).random((n, d)) >= 0.1) / 0.9).astype(np.float32)


def ladder_input(n, d, s):
    return base(n, d) * np.float32(s)


def mixed_inputs(n, d):
    """ordinary embeddings with tiny components: these must stay on the fp16 form"""
    b = base(n, d)
    out = {}
    Z = b.copy(); Z[0::2] *= np.float32(1e-5); Z[1::2] *= np.float32(100.0)
    out["rows_1e-5_100"] = Z
    Z = b * np.float32(0.7); Z[17] *= np.float32(1e-5); Z[:, 3] *= np.float32(1e-5)
    out["row_col_1e-5"] = Z
    rng = np.random.default_rng(n + d)
    u = rng.random((n, d))
    Z = b * np.float32(0.7)
    Z[u < 0.05] = 0.0
    tiny = (u >= 0.05) & (u < 0.10)
    Z[tiny] = np.where(rng.random((n, d)) < 0.5, np.float32(1e-7), np.float32(-1e-7))[tiny]
    out["zeros_1e-7"] = Z
    return out


def guard_positions(n, d):
    """(row, column) of the one large entry: the first row of a row panel (of either panel height) and the last
    valid row, which lies in a tail tile"""
    return [(256, 2), (n - 1, d - 1)]


def guard_input(n, d, v, pos):
    Z = base(n, d) * np.float32(0.7)
    Z[pos] = np.float32(v)
    return Z


def in_range_inputs(n, d):
    """name -> Z: every finite input of the GPU file that the kernel keeps on the fp16 form (max |Z| <= F16_MAX)"""
    out = {f"ladder_{s:g}": ladder_input(n, d, s) for s in LADDER}
    out.update(mixed_inputs(n, d))
    for v in GUARD_IN:
        for pos in guard_positions(n, d):
            out[f"guard_{v:g}@{pos[0]}"] = guard_input(n, d, v, pos)
    return out


def out_of_range_inputs(n, d):
    """name -> Z: the finite inputs that the range guard hands to the three-piece bf16 form"""
    return {f"guard_{v!r}@{pos[0]}": guard_input(n, d, v, pos) for v in GUARD_OUT for pos in guard_positions(n, d)}


# ----------------------------------------------------------------- pieces
def f16_pieces(v):
    """hi = fp16(v), lo = fp16(v - hi): their sum in fp64 (not finite beyond fp16's range: hi overflows)"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
        return hi.astype(np.float64) + lo.astype(np.float64)


def _bf16(v):
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def bf16_pieces(v, k):
    """the sum of k bf16 pieces, each the rounding of what the ones before left"""
    v = np.asarray(v, dtype=np.float32)
    rest, total = v.copy(), np.zeros(v.shape, np.float64)
    for _ in range(k):
        p = _bf16(rest)
        total += p.astype(np.float64)
        rest = rest - p
    return total


# ----------------------------------------------------------------- the loss in fp64 and its piece models
def _adjacency(src, dst, n):
    A = np.zeros((n, n))
    np.add.at(A, (dst, src), 1.0)
    return A


def _sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def _loss(S, A, pw):
    """mean of (1 - a) x + (1 + (pw - 1) a) softplus(-x)"""
    sp = np.maximum(-S, 0.0) + np.log1p(np.exp(-np.abs(S)))               # softplus(-x)
    return float(((1.0 - A) * S + (1.0 + (pw - 1.0) * A) * sp).mean())


class Problem:
    """one graph: adjacency, pos_weight and the exact fp64 loss / gradient of an embedding"""

    def __init__(self, n, src, dst):
        self.n = n
        self.A = _adjacency(src, dst, n)
        self.pw = (n * n - self.A.sum()) / self.A.sum()
        self.w = 1.0 + (self.pw - 1.0) * self.A
        self.er, self.ec = np.nonzero(self.A)
        self.ey = self.A[self.er, self.ec]

    def exact(self, Z, mask=None):
        """(loss, dZ) in fp64"""
        m = np.ones(Z.shape) if mask is None else mask.astype(np.float64)
        Zt = Z.astype(np.float64) * m
        S = Zt @ Zt.T
        G = self.w * _sigmoid(S) - self.pw * self.A
        return _loss(S, self.A, self.pw), ((G + G.T) @ Zt) / (self.n * self.n) * m

    def model(self, Z, mask=None, form="f16", centred=True):
        """(loss, dZ) with the operands of the matrix-pipe products replaced by their pieces.
        form "f16": two fp16 pieces everywhere; "bf16": three bf16 pieces for S, two for P and V (the kernel's
        three-piece form); "bf16x3": three bf16 pieces for everything (centred=False only: the table of the issue
        that asked for these tests)."""
        n = self.n
        m32 = np.ones(Z.shape, np.float32) if mask is None else mask.astype(np.float32)
        Zt32 = Z.astype(np.float32) * m32                     # the prepare step's fp32 product
        m, Zt = m32.astype(np.float64), Zt32.astype(np.float64)
        if form == "f16":
            split_s = split_v = split_p = f16_pieces
        else:
            split_s = lambda v: bf16_pieces(v, 3)
            split_v = split_p = (lambda v: bf16_pieces(v, 3)) if form == "bf16x3" else (lambda v: bf16_pieces(v, 2))
        rows = split_s(Zt32 * np.float32(LOG2E)) / LOG2E
        S = rows @ split_s(Zt32).T
        loss = _loss(S, self.A, self.pw)
        V = split_v(Zt32)
        if not centred:
            G = self.w * _sigmoid(S) - self.pw * self.A
            return loss, ((G + G.T) @ V) / (n * n) * m
        # P on the tiles at and right of the diagonal, mirrored; split like the kernel's P fragments
        P = split_p((_sigmoid(np.triu(S)) - 0.5).astype(np.float32))
        P = np.triu(P) + np.triu(P, 1).T
        # the edge walk, from the fp32 values themselves: E_ij = a_ij ((pw - 1) sigmoid(x_ij) - pw), (E + E^T) Zt
        er, ec = self.er, self.ec
        e = (self.ey * ((self.pw - 1.0) * _sigmoid(np.einsum("ij,ij->i", Zt[er], Zt[ec])) - self.pw))[:, None]
        edge = np.zeros(Zt.shape)
        np.add.at(edge, er, e * Zt[ec])
        np.add.at(edge, ec, e * Zt[er])
        dZt = 2.0 * (P @ V) + Zt.sum(axis=0)[None, :] + edge
        return loss, dZt / (n * n) * m


def errors(got, ref):
    """(loss error relative to max(1, |ref|), gradient error relative to max |ref|): the suite's two figures"""
    (l, g), (l0, g0) = got, ref
    return abs(l - l0) / max(1.0, abs(l0)), float(np.abs(g - g0).max() / np.abs(g0).max())
