"""numpy restatement of K17 (gae_decoder_bce_sampled), written from the contract in include/gae_hip_experimental.h:
the sampler bit for bit (Philox4x32-10 keys, 4-round Feistel with cycle walking) and the estimate with its gradient in
fp64.  Shared by tests/test_sampled_loss_cpu.py and tests/test_gpu_sampled_loss.py."""
import numpy as np

M32 = 0xFFFFFFFF
KEY_XOR = 0xD1B54A32D192ED03


def philox4x32_10(ctr, draw, seed):
    c = [ctr & M32, (ctr >> 32) & M32, draw & M32, (draw >> 32) & M32]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c


def _mask(w):
    return np.uint64((1 << w) - 1)


def _round(r, k):
    """F(R, k) on uint64 arrays holding uint32 values"""
    x = (r ^ np.uint64(k)) & np.uint64(M32)
    x = (x * np.uint64(0x9E3779B1)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    x ^= x >> np.uint64(13)
    return x


class Perm:
    """a keyed bijection of [0, n)"""

    def __init__(self, keys, n):
        self.k, self.n = [int(k) for k in keys], int(n)
        b = 0
        while (1 << b) < n:
            b += 1
        h = b >> 1
        self.wl, self.wr = b - h, h

    def enc(self, v):
        v = np.asarray(v, np.uint64).copy()
        wl, wr = self.wl, self.wr
        for q in range(4):
            L, R = v >> np.uint64(wr), v & _mask(wr)
            v = (R << np.uint64(wl)) | (L ^ (_round(R, self.k[q]) & _mask(wl)))
            wl, wr = wr, wl
        return v

    def dec(self, v):
        v = np.asarray(v, np.uint64).copy()
        for q in (3, 2, 1, 0):
            wl, wr = (self.wr, self.wl) if q & 1 else (self.wl, self.wr)
            R, X = v >> np.uint64(wl), v & _mask(wl)
            L = X ^ (_round(R, self.k[q]) & _mask(wl))
            v = (L << np.uint64(wr)) | R
        return v

    def _walk(self, step, i):
        v = step(i)
        while True:
            bad = v >= np.uint64(self.n)
            if not bad.any():
                return v.astype(np.int64)
            v[bad] = step(v[bad])

    def fwd(self, i):
        return self._walk(self.enc, i)

    def inv(self, y):
        return self._walk(self.dec, y)


def sampler(seed, t, n):
    """(sigma, tau) of draw t"""
    seed = int(seed) ^ KEY_XOR
    t = int(t) & ((1 << 64) - 1)
    return Perm(philox4x32_10(0, t, seed), n), Perm(philox4x32_10(1, t, seed), n)


def partners(seed, t, n, m, rows):
    """pi_s(r) for r in ``rows`` (global ids), s < m: int64 [len(rows), m]"""
    sig, tau = sampler(seed, t, n)
    rows = np.asarray(rows, np.int64)
    o = tau.fwd(np.arange(m, dtype=np.uint64))
    sr = sig.fwd(rows.astype(np.uint64))
    return sig.inv(((sr[:, None] + o[None, :]) % n).astype(np.uint64))


def inverse_partners(seed, t, n, m, cols):
    """i with pi_s(i) = j, for j in ``cols``: int64 [len(cols), m]"""
    sig, tau = sampler(seed, t, n)
    cols = np.asarray(cols, np.int64)
    o = tau.fwd(np.arange(m, dtype=np.uint64)).astype(np.int64)
    sj = sig.fwd(cols.astype(np.uint64)).astype(np.int64)
    return sig.inv(((sj[:, None] - o[None, :]) % n).astype(np.uint64))


def _sp(x):
    return np.logaddexp(0.0, x)


def _sig(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def estimate(Zt, csr, csc, pw, seed, t, m, row_begin=0, n_local=None, part=None):
    """fp64 (Lhat share, dLhat/dZt) of the rows [row_begin, row_begin + n_local), as the kernel defines them: the share
    holds the rows' own edges and samples, the gradient rows are those of the GLOBAL estimate (own edges, transposed
    edges, own samples, inverse partners).  ``csr`` / ``csc``: (indptr, indices) of the local rows of A / A^T, global
    column ids.  ``part``: the rows' partners [n_local, m] (None: from the sampler)."""
    Zt = np.asarray(Zt)
    n = Zt.shape[0]
    n_local = n - row_begin if n_local is None else n_local
    rows = np.arange(row_begin, row_begin + n_local)
    if part is None:
        part = partners(seed, t, n, m, rows)
    inv = inverse_partners(seed, t, n, m, rows)
    w = n / m

    def z(idx):                                              # gathered rows in fp64 (Zt itself may be huge)
        return Zt[idx].astype(np.float64)
    ip, ix = (np.asarray(a, np.int64) for a in csr)
    tp, tx = (np.asarray(a, np.int64) for a in csc)
    zr = z(rows)
    er = np.repeat(np.arange(n_local), np.diff(ip))          # local row of every edge
    ze = z(ix[ip[0]:ip[-1]])
    x = np.einsum("ij,ij->i", zr[er], ze)
    loss = (pw * _sp(-x) - _sp(x)).sum()
    g = np.zeros((n_local, Zt.shape[1]))
    np.add.at(g, er, (-pw * _sig(-x) - _sig(x))[:, None] * ze)
    tr = np.repeat(np.arange(n_local), np.diff(tp))
    zt = z(tx[tp[0]:tp[-1]])
    xt = np.einsum("ij,ij->i", zr[tr], zt)
    np.add.at(g, tr, (-pw * _sig(-xt) - _sig(xt))[:, None] * zt)
    zp = z(part)
    xs = np.einsum("rk,rsk->rs", zr, zp)
    loss += w * _sp(xs).sum()
    g += np.einsum("rs,rsk->rk", w * _sig(xs), zp)
    zi = z(inv)
    xi = np.einsum("rk,rsk->rs", zr, zi)
    g += np.einsum("rs,rsk->rk", w * _sig(xi), zi)
    return loss / n ** 2, g / n ** 2


def csr_of(rows_of_edges, cols_of_edges, n_rows, row_begin=0):
    """(indptr, indices) int32 of the rows [row_begin, row_begin + n_rows), stable in edge order"""
    r = np.asarray(rows_of_edges, np.int64) - row_begin
    c = np.asarray(cols_of_edges, np.int64)
    keep = (r >= 0) & (r < n_rows)
    r, c = r[keep], c[keep]
    order = np.argsort(r, kind="stable")
    ip = np.zeros(n_rows + 1, np.int64)
    np.add.at(ip, r + 1, 1)
    return np.cumsum(ip).astype(np.int32), c[order].astype(np.int32)


def exact_loss(Zt, src, dst, pw):
    """the reference loss, fp64 (small n only)"""
    Zt = np.asarray(Zt, np.float64)
    n = Zt.shape[0]
    X = Zt @ Zt.T
    Y = np.zeros((n, n))
    np.add.at(Y, (np.asarray(dst), np.asarray(src)), 1.0)
    L = (1 - Y) * X + (1 + (pw - 1) * Y) * _sp(-X)
    G = ((1 - Y) - (1 + (pw - 1) * Y) * _sig(-X)) / n ** 2
    return L.mean(), (G + G.T) @ Zt
