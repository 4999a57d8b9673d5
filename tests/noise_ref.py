"""numpy restatement of the stochastic half of the VGAE step, written from the contract in include/gae_hip.h and
include/gae_hip_experimental.h (no kernel code is imported): the Philox4x32-10 words of gae_dropout_mask and
gae_normal_noise bit for bit, the fp32 uniforms of the noise exactly as the kernel forms them, Box-Muller and the VGAE
head (gae_vgae_head_fwd / _bwd / gae_x_vgae_head_prep) in float64, and a rounding bound per output element derived from
the fp32 operation sequence of the kernels.  Shared by tests/test_noise_ref_cpu.py, tests/test_gpu_noise.py and
tests/test_gpu_vgae_head.py.

Assumptions the bounds rest on (a GPU run that contradicts one is a finding, not a constant to widen):
  * __expf(l) has a relative error of at most (|l| + 2) 2^-23: one rounding of l log2(e), which the exponential
    amplifies by |l|, plus the rounding of the exponential instruction itself (EXP_REL);
  * fmaf rounds once; every other fp32 operation rounds once, whether or not the compiler contracts a product and a sum
    (a contraction only removes a rounding the bound has counted);
  * sums of the KL bracket run in fp64 (their own error is counted with 2^-53 per addition).
The fast log / sin / cos of the noise are not correctly rounded and their error constants are not documented, so the
noise bound is NOISE_A rad + NOISE_B |z| with the two constants set from a measurement (MEASUREMENTS.md, "VGAE head and
random draws"): 4 x the largest |gpu - ref| / (rad + |z|) seen on the device."""
import numpy as np

import bf16_ref

M32 = 0xFFFFFFFF
U24 = 2.0 ** -24                      # unit roundoff of fp32
U53 = 2.0 ** -53
TINY = 2.0 ** -149                    # one fp32 subnormal step: the floor of every bound
NOISE_TAG = 0x6E6F726D                # "norm": word 2 of the noise counter, XORed with the high half of the draw index
TWO_PI_F32 = np.float32(6.28318530717958648)
# measured on gfx950: worst |gpu - ref| / (rad + |z|) = 4.50e-7 over the cases of tests/test_gpu_noise.py (2 097 157
# elements at four (offset, draw) pairs, the short sizes at all twelve); both constants are 4 x that (MEASUREMENTS.md)
NOISE_MEASURED = 4.50e-7
NOISE_A = 4 * NOISE_MEASURED          # per unit of rad = sqrt(-2 ln u1): the absolute error of the fast sin / cos
NOISE_B = 4 * NOISE_MEASURED          # per unit of |z|: the relative error of rad (fast log, sqrtf) and of the product


def _u64(x):
    return np.uint64(int(x) & 0xFFFFFFFFFFFFFFFF)


# ------------------------------------------------------------------ Philox4x32-10
def philox_words(ctr, c2, c3, seed):
    """uint32 [len(ctr), 4]: Philox4x32-10 of the counters {ctr low, ctr high, c2, c3} under the key
    {seed low, seed high}.  `ctr`: uint64 array; c2, c3: 32-bit words; seed: 64 bits."""
    ctr = np.asarray(ctr, np.uint64).reshape(-1)
    m = np.uint64(M32)
    s32 = np.uint64(32)
    c0, c1 = ctr & m, ctr >> s32
    c2 = np.full(ctr.shape, int(c2) & M32, np.uint64)
    c3 = np.full(ctr.shape, int(c3) & M32, np.uint64)
    k0, k1 = int(seed) & M32, (int(seed) >> 32) & M32
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


def _counters(n_elems, offset):
    """the counter of every block of four elements: offset + q, modulo 2^64"""
    nq = (int(n_elems) + 3) // 4
    with np.errstate(over="ignore"):
        return _u64(offset) + np.arange(nq, dtype=np.uint64)


# ------------------------------------------------------------------ dropout
def dropout_of_words(words, p):
    """the multiplier of each 32-bit draw: u = float32(word >> 8) 2^-24, kept iff u >= float32(p), kept value
    float32(1) / (float32(1) - float32(p))"""
    p = np.float32(p)
    u = (np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(U24)
    scale = np.float32(1) / (np.float32(1) - p)
    return np.where(u >= p, scale, np.float32(0)).astype(np.float32)


def dropout_mask(n_elems, p, seed, offset=0, draw=0):
    """gae_dropout_mask: fp32 [n_elems].  Block q of four elements uses counter offset + q in words 0 / 1 and the draw
    index in words 2 (low) / 3 (high); element 4 q + i takes output word i."""
    draw = int(draw) & 0xFFFFFFFFFFFFFFFF
    w = philox_words(_counters(n_elems, offset), draw & M32, draw >> 32, seed)
    return dropout_of_words(w.reshape(-1)[:int(n_elems)], p)


# ------------------------------------------------------------------ normal noise
def u1_of_words(words):
    """(float32(word >> 8) + 0.5f) 2^-24 in fp32.  The sum rounds to even from 2^23 on: the grid above 0.5 is twice
    as coarse and the top word gives exactly 1, so u1 lies in (0, 1] with 2^-25 its smallest value."""
    x = (np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32)
    return ((x + np.float32(0.5)) * np.float32(U24)).astype(np.float32)


def u2_of_words(words):
    """float32(word >> 8) 2^-24: [0, 1), exact"""
    return ((np.asarray(words, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(U24)).astype(np.float32)


def noise_words(n_elems, seed, offset=0, draw=0):
    """uint32 [ceil(n / 4), 4] of gae_normal_noise: counter offset + q in words 0 / 1, the tag XOR the HIGH half of
    the draw index in word 2, the LOW half in word 3"""
    draw = int(draw) & 0xFFFFFFFFFFFFFFFF
    return philox_words(_counters(n_elems, offset), NOISE_TAG ^ (draw >> 32), draw & M32, seed)


def normal_uniforms(n_elems, seed, offset=0, draw=0):
    """(u1, u2) fp32 [n_elems] of every element's half of its block: elements 4 q + 2 h and 4 q + 2 h + 1 share
    u1 from output word 2 h and u2 from word 2 h + 1"""
    w = noise_words(n_elems, seed, offset, draw)
    u1 = np.repeat(u1_of_words(w[:, 0::2]).reshape(-1), 2)[:int(n_elems)]
    u2 = np.repeat(u2_of_words(w[:, 1::2]).reshape(-1), 2)[:int(n_elems)]
    return u1, u2


def box_muller(u1, u2, odd):
    """float64 (z, rad) on fp32 uniforms: rad = sqrt(-2 ln u1), the angle float32(2 pi_f32 * u2) taken to fp64, cos for
    the even element of a pair and sin for the odd one"""
    u1, u2 = np.asarray(u1, np.float32), np.asarray(u2, np.float32)
    rad = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    ang = (TWO_PI_F32 * u2).astype(np.float32).astype(np.float64)
    return rad * np.where(odd, np.sin(ang), np.cos(ang)), rad


def normal_noise(n_elems, seed, offset=0, draw=0):
    """gae_normal_noise: (ref fp64 [n_elems], bound).  bound = NOISE_A rad + NOISE_B |z|: 0 where u1 == 1 (rad = 0: the
    kernel must give an exact zero there)"""
    u1, u2 = normal_uniforms(n_elems, seed, offset, draw)
    z, rad = box_muller(u1, u2, (np.arange(int(n_elems)) & 1) == 1)
    return z, NOISE_A * rad + NOISE_B * np.abs(z)


# ------------------------------------------------------------------ the VGAE head
def _f64(x):
    return np.asarray(x, np.float64)


def exp_rel(l):
    """the assumed relative error of __expf(l) (module docstring)"""
    return (np.abs(_f64(l)) + 2.0) * 2.0 ** -23


def _bracket(mu, ls):
    """(b, bound) of the fp32 KL bracket 1 + 2 l - m m - s s, s = __expf(l), per element.  At most five roundings
    (1 + 2l, m m, the difference, s s, the difference), each of a value no larger than T = 1 + 2 |l| + m^2 + s^2 grown by
    the earlier ones, plus the error of s^2 itself: s = e^l (1 + r), |r| <= exp_rel."""
    m, l = _f64(mu), _f64(ls)
    s2 = np.exp(2.0 * l)
    r = exp_rel(l)
    ds2 = s2 * (2.0 * r + r * r)
    T = 1.0 + 2.0 * np.abs(l) + m * m + s2 + ds2
    return 1.0 + 2.0 * l - m * m - s2, 5.0 * U24 * T * (1.0 + 2.0 ** -20) + ds2 + TINY


def _kl_of(bsum, bsum_abs, bound_sum, count, n):
    """(kl, bound) of float32(scale * fp64 sum): the brackets' own bounds, count fp64 additions, the final rounding"""
    scale = 0.5 / (float(n) * float(n))
    kl = -scale * bsum
    err = scale * (bound_sum + (count + 2) * U53 * (bsum_abs + bound_sum))
    return kl, err + U24 * (abs(kl) + err) + TINY


def head_fwd(mu, ls, eps):
    """gae_vgae_head_fwd on [n, d] operands: (z64, kl64, z_bound, kl_bound).
    z = fmaf(eps, s, m): |eps| e^l exp_rel from s, then one rounding of the result.
    KL = -0.5 / n^2 sum (1 + 2 l - m^2 - e^{2 l}): fp32 brackets (see _bracket) summed in fp64, one fp32 rounding."""
    m, l, e = _f64(mu), _f64(ls), _f64(eps)
    n = m.shape[0]
    s = np.exp(l)
    z = m + e * s
    dz = np.abs(e) * s * exp_rel(l)
    z_bound = dz + U24 * (np.abs(z) + dz) + TINY
    b, bb = _bracket(m, l)
    kl, kl_bound = _kl_of(b.sum(), np.abs(b).sum(), bb.sum(), b.size, n)
    return z, kl, z_bound, kl_bound


def head_bwd(dz, mu, ls, eps, gkl, n):
    """gae_vgae_head_bwd: (dmu64, dls64, (dmu_bound, dls_bound)); dz None = 0, gkl None = 1.
    gk = fl(gkl * fl(1 / n^2)): two roundings.  dmu = fmaf(gk, m, g).  dls = fmaf(fl(g eps), s, fl(gk * fl(s s - 1)))
    with s = __expf(l)."""
    m, l, e = _f64(mu), _f64(ls), _f64(eps)
    g = np.zeros_like(m) if dz is None else _f64(dz)
    gk = (1.0 if gkl is None else float(gkl)) / (float(n) * float(n))
    eg = 2.0 * U24 + U24 * U24                                   # relative error of gk
    dmu = g + gk * m
    e_dmu = np.abs(gk * m) * eg
    dmu_bound = e_dmu + U24 * (np.abs(dmu) + e_dmu) + TINY
    s = np.exp(l)
    r = exp_rel(l)
    q = s * s - 1.0
    ds2 = s * s * (2.0 * r + r * r)                              # s s against e^{2 l}
    e_q = ds2 + U24 * (s * s + ds2)                              # ... rounded (absent when contracted into an fma)
    e_q = e_q + U24 * (np.abs(q) + e_q)                          # ... minus one, rounded
    p = gk * q
    e_p = abs(gk) * (1.0 + eg) * e_q + abs(gk) * eg * np.abs(q)
    e_p = e_p + U24 * (np.abs(p) + e_p)                          # the product, rounded
    t = g * e * s
    e_t = np.abs(t) * (U24 + r + U24 * r)                        # fl(g eps) times s
    dls = t + p
    dls_bound = e_t + e_p + U24 * (np.abs(dls) + e_t + e_p) + TINY
    return dmu, dls, (dmu_bound, dls_bound)


def bf16_split(z32):
    """(hi, lo) uint16 bit patterns of the fused loss's operand split: hi = bf16(z), lo = bf16(z - hi), both
    round-to-nearest-even; z - hi is exact in fp32"""
    z = np.asarray(z32, np.float32).astype(np.float64)
    hi = bf16_ref.rne_bf16(z)
    lo = (z - hi).astype(np.float32).astype(np.float64)
    return bf16_ref.bf16_bits(hi), bf16_ref.bf16_bits(lo)


def block_colsums(z32, rows_per_block=64):
    """(sums, bound) fp64 [blocks, d]: the column sums of every block of 64 rows of the fp32 z that was written, and
    64 2^-53 sum |z|: what any order of 64 fp64 additions stays within"""
    z = np.asarray(z32, np.float32).astype(np.float64)
    n, d = z.shape
    blocks = (n + rows_per_block - 1) // rows_per_block
    pad = np.zeros((blocks * rows_per_block, d))
    pad[:n] = z
    pad = pad.reshape(blocks, rows_per_block, d)
    return pad.sum(1), rows_per_block * U53 * np.abs(pad).sum(1)


def head_prep(mu, ls, eps):
    """gae_x_vgae_head_prep (d = 16) on [n, 16] operands, as a dict:
      z, z_bound            as head_fwd (the kernel's z must also equal gae_vgae_head_fwd's bit for bit, and Zt == z);
      blocks                ceil(n / 64);
      kl_partial, kl_partial_bound   [blocks]: the fp64 sum of the block's fp32 brackets, unscaled;
      kl, kl_bound          what sum_b kl_partial[b] * (-0.5 / n^2) must meet (the bound of kl_out before its fp32 rounding
                            is inside kl_bound).
    Zhi / Zlo and the column sums are functions of the fp32 z that was written: bf16_split, block_colsums."""
    m, l = _f64(mu), _f64(ls)
    n, d = m.shape
    assert d == 16
    z, kl, z_bound, kl_bound = head_fwd(mu, ls, eps)
    blocks = (n + 63) // 64
    b, bb = _bracket(m, l)
    klp, klb = np.zeros(blocks), np.zeros(blocks)
    for k in range(blocks):
        rows = slice(64 * k, min(64 * k + 64, n))
        cnt = b[rows].size
        klp[k] = b[rows].sum()
        klb[k] = bb[rows].sum() + (cnt + 2) * U53 * (np.abs(b[rows]).sum() + bb[rows].sum())
    return dict(z=z, z_bound=z_bound, blocks=blocks, kl_partial=klp, kl_partial_bound=klb, kl=kl, kl_bound=kl_bound)


# ------------------------------------------------------------------ comparison
def worst(got, ref, bound):
    """(ratio, index): the largest |got - ref| / bound and its flat index.  bound == 0 admits only got == ref; a NaN
    in `got` counts as infinitely wrong."""
    got, ref = _f64(got).reshape(-1), _f64(ref).reshape(-1)
    bound = np.broadcast_to(_f64(bound), ref.shape) if np.ndim(bound) == 0 else _f64(bound).reshape(-1)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0, -1
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(got), np.inf, ratio)
    i = int(np.argmax(ratio))
    return float(ratio[i]), i
