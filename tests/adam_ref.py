"""Reference for K12 (gae_adam_step, csrc/optim.hip), numpy only: the library's one order for adding a partial-sum
list (written from the contract in DESIGN.md / csrc/common.h, not from the kernel), the layout of such a list in
memory, one Adam step in float64, and the case tables that tests/test_adam_ref_cpu.py and tests/test_gpu_adam_abi.py
share."""
import functools
import math

import numpy as np

GUARD = 64               # floats in front of and behind every buffer a test hands to a launch
U24 = 2.0 ** -24         # unit roundoff of fp32

# ------------------------------------------------------------------ case tables
# list lengths on both sides of every point where the code changes form: 7 | 8 (1024 / 256 elements per block),
# 16 | 17 (the 16 loads in flight), 32 | 33 (one lane / 64 lanes per element), 64 | 65 (every lane has one / a second
# partial), 1024 | 1025 (a second trip of the 64-lane loop)
LIST_LENGTHS = [1, 2, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1100]
SIZES_SHORT = [1, 3, 255, 256, 257, 1023, 1024, 1025, 1030]     # lists of <= 32 partials: tails of 256 / 1024 per block
SIZES_LONG = [1, 3, 4, 5, 9, 257]                               # longer lists: tails of 4 per block
LAYOUTS = ["dense", "padded_rows", "row_len_1"]
N_DRAW = max(SIZES_SHORT)
INPUT_SEED = 20240607    # picked once; test_adam_ref_cpu.py asserts what the GPU test needs of these inputs

# (n, n_partials) of the mixed launch: the tensor lookup crosses every kind
MIXED = [(1030, 0), (0, 0), (257, 3), (5, 33), (1, 0), (1025, 8), (300, 32), (9, 200), (0, 5), (1024, 0), (256, 17),
         (4, 64), (3, 1025), (2049, 7), (255, 16), (1, 1)]
ALL_EMPTY = [(0, 0), (0, 3), (0, 0), (0, 5)]
EDGE_BETAS = [(0.0, 0.0), (0.5, 0.9), (0.9, 0.999)]
WEIGHT_DECAYS = [0.0, 1e-2]
TRAJECTORY_BOUND = 2e-6  # the project's bound for an Adam trajectory (test_gpu_parity.py::test_adam_matches_torch)


def sizes_for(n_partials):
    return SIZES_SHORT if n_partials <= 32 else SIZES_LONG


def layout(kind, n):
    """(stride, row_len, row_pitch) of a list of n-element partials in one of the three layouts"""
    if kind == "dense":
        return max(n, 1), max(n, 1), max(n, 1)
    if kind == "padded_rows":
        rows = (n + 4) // 5
        return rows * 8 + 24, 5, 8
    if kind == "row_len_1":
        return n * 3 + 5, 1, 3
    raise ValueError(kind)


# ------------------------------------------------------------------ the order
def sum_in_library_order(P):
    """fp32 sums of the fp32 list P [n_partials, n] in the library's order, rounded to fp32 after every add:
    up to 32 partials 0, 1, 2, ... in order from +0; longer lists as 64 lane sums (lane l adds l, l + 64, ... in
    order), then lane[i] += lane[i + off] for off = 32, 16, ..., 1, and lane 0 is the result"""
    P = np.asarray(P)
    assert P.dtype == np.float32 and P.ndim == 2
    n_partials, n = P.shape
    if n_partials <= 32:
        g = np.zeros(n, np.float32)
        for q in range(n_partials):
            g = g + P[q]
        assert g.dtype == np.float32
        return g
    lanes = np.zeros((64, n), np.float32)
    for q in range(n_partials):          # ascending q keeps every lane's own order l, l + 64, ...
        lanes[q % 64] = lanes[q % 64] + P[q]
    off = 32
    while off:
        lanes[:off] = lanes[:off] + lanes[off:2 * off]
        off //= 2
    assert lanes.dtype == np.float32
    return lanes[0].copy()


def sum_depth(n_partials):
    """dependent roundings on the longest path of the order above"""
    return n_partials if n_partials <= 32 else -(-n_partials // 64) + 6


def sum_bound(P):
    """|fp32 sum in that order - exact sum| <= depth 2^-24 sum |p_q| per element (the standard bound for a chain of
    `depth` roundings)"""
    P = np.asarray(P, np.float64)
    return sum_depth(P.shape[0]) * U24 * np.abs(P).sum(0)


# ------------------------------------------------------------------ the layout
def partial_index(n_partials, n, stride, row_len, row_pitch):
    """[n_partials, n] offsets: element e of partial q sits at q stride + (e // row_len) row_pitch + e % row_len"""
    e = np.arange(n, dtype=np.int64)
    q = np.arange(n_partials, dtype=np.int64)[:, None]
    return q * stride + (e // row_len) * row_pitch + e % row_len


def place_partials(P, stride, row_len, row_pitch, fill=np.nan):
    """the flat fp32 buffer that holds the list P [n_partials, n] in that layout, GUARD floats in front of the list
    and behind it; every float that is not an element of the list -- row padding, gaps between partials, the guards --
    is `fill` (NaN: any read outside the list poisons the sum).  The list starts at buffer[GUARD]."""
    P = np.asarray(P, np.float32)
    n_partials, n = P.shape
    idx = partial_index(n_partials, n, stride, row_len, row_pitch)
    span = int(idx.max()) + 1 if idx.size else 0
    assert np.unique(idx).size == idx.size, "layout overlaps itself"
    buf = np.full(GUARD + span + GUARD, fill, np.float32)
    buf[GUARD + idx] = P
    return buf


# ------------------------------------------------------------------ the update rule
def f32(x):
    """the value a `float` argument of the C ABI receives"""
    return float(np.float32(x))


def adam_fp64(p, g, m, v, t, lr, b1, b2, eps, wd):
    """one step of the rule in include/gae_hip.h in float64, t 1-based -> (p, m, v).  Pass the hyper-parameters the
    call receives (f32(x) of each): the ABI takes `float` and the kernel widens those values."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr / (1.0 - b1 ** t) * (m / (np.sqrt(v) / math.sqrt(1.0 - b2 ** t) + eps))
    return p, m, v


def rel_err(a, b):
    """tests/test_gpu_parity.py::rel_err: max abs difference over max(1, max |reference|)"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    if b.size == 0:
        return 0.0
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _wide_draw(n_partials):
    rng = np.random.default_rng([INPUT_SEED, n_partials])
    P = rng.standard_normal((n_partials, N_DRAW)) * 10.0 ** rng.uniform(-3.0, 3.0, (n_partials, N_DRAW))
    P = P.astype(np.float32)
    P.setflags(write=False)
    return P


def wide_partials(n_partials, n):
    """N(0, 1) 10^U(-3, 3): the first n elements of ONE draw per list length, so that what test_adam_ref_cpu.py asserts
    of the draw (it tells the orders apart, every partial counts) holds for the lists the GPU test sums"""
    return _wide_draw(n_partials)[:, :n]
