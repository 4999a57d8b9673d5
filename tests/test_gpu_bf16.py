"""bf16-stored SpMM held to its rounding contract (tests/bf16_ref.py): fp32 accumulation, ONE round-to-nearest-even
rounding per output element (GAE_SPMM_ACCUMULATE: the old bf16 value added in fp32 before it), in every launch form of
gae_spmm_csr that stores bf16 -- row-group kernels v1 / v2, packed tables of 4 / 8 / 16 slots (the ell kernels and the
row-group kernel reading the table; rows longer than the table gathered by the whole wave), the skew plan (single-
segment rows written by the segment kernel, longer rows through spmm_combine_kernel; with and without the light-row
list), XCD-pinned ("homed") rows through spmm_vh_combine_kernel, XCD feature tiles, row / column scales, both
directions (CSR of A and of A^T), padded and unpadded rows with NaN in the pad columns.

Exact inputs (integers in [-127, 127] times a power of two, power-of-two scales): every fp32 partial sum is exact in any
order, so the output equals rne_bf16(fp64 sum) bit for bit -- sums of 9+ significant bits, so ties occur.  Random
inputs: every element lies in its bf16 bracket.  Special rows: a NaN row reaches every row that gathers it, sums beyond
the largest finite bf16 (an exact tie at its top included) give +-Inf, a row without edges and an exact cancellation
are +0."""
import os
import sys
from contextlib import contextmanager

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BIG = 127.0 * 2.0 ** 120                        # two of them: 254 * 2^120 < largest bf16 (255 * 2^120)
# special rows (as gathered in the CSR of A): row -> column ids; special columns (H rows) below
SPECIAL_COLS = {1: np.nan, 2: BIG, 3: -BIG, 4: 1.5 * 2.0 ** 120, 6: -1.5 * 2.0 ** 120, 7: 1.25 * 2.0 ** 120}
SPECIAL_ROWS = {0: [2, 2],                      # 254 * 2^120: finite
                8: [2, 2, 4],                   # 255.5 * 2^120: exact tie with 2^128 -> +Inf (even)
                9: [2, 2, 2],                   # beyond fp32: +Inf
                11: [3, 3, 6],                  # -Inf
                12: [1, 10, 15],                # NaN row
                13: [2, 3],                     # exact cancellation: +0
                14: [2, 2, 7]}                  # 255.25 * 2^120: the largest finite bf16
EMPTY = 5                                       # no in- or out-edges
LONG = (300, 130, 65, 40, 17, 9)                # rows (and columns) of these lengths: homed, multi- and single-segment


@contextmanager
def knobs(**kv):
    from gae_dgl_amd import _lib
    import ctypes
    saved = []
    try:
        for k, v in kv.items():
            old = ctypes.c_int64(0)
            _lib.call("gae_tuning_get", k.encode(), ctypes.byref(old))
            saved.append((k, old.value))
            _lib.call("gae_tuning_set", k.encode(), int(v))
        yield
    finally:
        for k, v in reversed(saved):
            _lib.call("gae_tuning_set", k.encode(), v)


def bf16_graph(n, rng):
    """random multigraph on nodes 16.., rows / columns of LONG lengths, the special rows on nodes 0..15"""
    e = 4 * n
    src = rng.integers(16, n, e); dst = rng.integers(16, n, e)
    for k, L in enumerate(LONG):
        a = 16 + 10 * k
        src = np.concatenate([src, rng.choice(np.arange(16, n), L, replace=False)]); dst = np.concatenate([dst, np.full(L, a)])
        dst = np.concatenate([dst, rng.choice(np.arange(16, n), L, replace=False)]); src = np.concatenate([src, np.full(L, a + 5)])
    for r, cols in SPECIAL_ROWS.items():
        src = np.concatenate([src, cols]); dst = np.concatenate([dst, np.full(len(cols), r)])
    return src.astype(np.int64), dst.astype(np.int64)


# (name, knobs, plan, scattered); plans: None, packed tables "t16" / "t8" / "t4", skew plans, the homed plan
FORMS = [("rowgroup2", {}, None, False), ("rowgroup1", {"spmm_variant": 1}, None, False),
         ("rowgroup2-rpg2", {"spmm_rpg": 2}, None, False),
         ("table16", {}, "t16", False), ("table16-rowgroup", {"spmm_ell": 2}, "t16", False),
         ("table8", {}, "t8", False), ("table4", {}, "t4", False),
         ("skew", {}, "skew", False), ("skew-nolist", {"spmm_light": 0}, "skew", False),
         ("skew-table", {}, "skew_t", False), ("homed", {}, "homed", False),
         ("tiles", {"spmm_tile_vecs": 8}, None, False), ("tiles-table", {"spmm_tile_vecs": 8}, "t16", False),
         ("scattered", {}, "t16", True), ("scattered-skew", {}, "skew", True)]
HEAVY = ("skew", "skew_t", "homed")


def plans_of(ip, ix, n):
    from gae_dgl_amd import ops
    p = {None: None}
    for w in (16, 8, 4):
        p[f"t{w}"] = ops.spmm_plan(ip, indices=ix, ell=True, threshold=10 ** 6, ell_width=w)
        assert p[f"t{w}"].ell is not None and p[f"t{w}"].n_heavy == 0
    p["skew"] = ops.spmm_plan(ip, threshold=8, segment=64)
    p["skew_t"] = ops.spmm_plan(ip, threshold=8, segment=64, indices=ix)
    assert p["skew"].n_heavy > 0 and p["skew_t"].ell is not None
    p["homed"] = ops.spmm_plan(ip, threshold=8, segment=128, indices=ix, ell=False, hot=False, n_cols=n, homed=True)
    assert p["homed"].homed is not None
    return p


def bf16_matrix(vals, ld, dev):
    """[n, F] bf16 view of a buffer of ``ld`` columns whose pad columns hold NaN"""
    n, F = vals.shape
    buf = torch.full((n, ld), float("nan"), dtype=torch.bfloat16, device=dev)
    buf[:, :F] = torch.from_numpy(np.ascontiguousarray(vals)).to(dev).to(torch.bfloat16)
    return buf[:, :F]


def check_spmm_bf16(F, exact, seed):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(seed)
    n = 700
    src, dst = bf16_graph(n, rng)
    s = 2.0 ** int(rng.integers(-6, 3))                  # power of two of the exact inputs
    ld = ops.padded_ld(F, torch.bfloat16)
    for transposed in (False, True):
        rows, cols = (src, dst) if transposed else (dst, src)
        ip, ix = ops.csr_from_coo(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), n, n)
        ipn, ixn = ip.cpu().numpy(), ix.cpu().numpy()
        plans = plans_of(ip, ix, n)
        if exact:
            Hv = rng.integers(-127, 128, (n, F)).astype(np.float64) * s
            old = rng.integers(-127, 128, (n, F)).astype(np.float64) * s
            rs = 2.0 ** rng.integers(-3, 4, n).astype(np.float64); cs = 2.0 ** rng.integers(-3, 4, n).astype(np.float64)
        else:
            Hv = R.rne_bf16(rng.standard_normal((n, F)) * np.exp(rng.standard_normal((n, 1)) * 2))
            old = R.rne_bf16(rng.standard_normal((n, F)) * 4)
            deg = np.maximum(np.bincount(rows, minlength=n), 1)
            rs = cs = (deg ** -0.5).astype(np.float32).astype(np.float64)
        if not transposed:                               # special columns / rows: unit scales, no old value
            for c, v in SPECIAL_COLS.items():
                Hv[c] = v
            cs = cs.copy(); cs[list(SPECIAL_COLS)] = 1.0
            rs = rs.copy(); rs[list(SPECIAL_ROWS)] = 1.0
            old[list(SPECIAL_ROWS)] = 0.0
        assert np.diff(ipn)[EMPTY] == 0
        H_pad = bf16_matrix(Hv, ld, DEV)                 # 16-byte rows, NaN pad: vector path
        H_flat = torch.from_numpy(Hv).to(DEV).to(torch.bfloat16)   # ld = F: scalar path unless F % 8 == 0
        rsd = torch.from_numpy(rs.astype(np.float32)).to(DEV); csd = torch.from_numpy(cs.astype(np.float32)).to(DEV)
        combos = [(False, False), (True, False), (False, True), (True, True)] if exact else [(False, False), (True, True)]
        for scaled, accumulate in combos:
            ref, asum, k = R.spmm64(ipn, ixn, Hv, rs if scaled else None, cs if scaled else None,
                                    old if accumulate else None)
            want = R.bf16_bits(ref)
            nan = np.isnan(ref)
            bracket = None if exact else R.bf16_bracket(ref, R.fp32_sum_bound(asum, k))
            for name, kv, pk, scattered in FORMS:
                if pk in HEAVY and F <= 24:
                    continue                             # (a skew plan needs F > 24 on the bf16 vector path)
                if name.startswith("tiles") and F <= 128:
                    continue                             # (feature tiles: rows of more than 16 vectors)
                layouts = ("pad", "flat") if name in ("rowgroup2", "rowgroup1", "table16", "skew") else ("pad",)
                for lay in layouts:
                    H = H_pad if lay == "pad" else H_flat
                    out = None
                    if accumulate:
                        out = bf16_matrix(old, ld, DEV)
                    with knobs(**kv):
                        got = ops.spmm_raw(ip, ix, H, n, rsd if scaled else None, csd if scaled else None, out=out,
                                           plan=plans[pk], scattered=scattered, accumulate=accumulate)
                    what = (F, exact, transposed, scaled, accumulate, name, lay)
                    if accumulate:
                        pad = R.tensor_bits(out.as_strided((n, ld), (ld, 1))[:, F:])
                        assert np.isnan(R.from_bits(pad)).all(), (what, "pad columns written")
                    gb = R.tensor_bits(got)
                    assert gb[EMPTY].tolist() == R.bf16_bits(old[EMPTY] if accumulate else np.zeros(F)).tolist(), \
                        (what, "row without edges")
                    assert np.array_equal(np.isnan(R.from_bits(gb)), nan), (what, "NaN pattern")
                    if exact:
                        bad = (gb != want) & ~nan
                        assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:3].tolist(),
                                               R.from_bits(gb[bad][:3]).tolist(), ref[bad][:3].tolist())
                    else:
                        R.assert_in_bracket(gb, ref, None, str(what), bracket=bracket)
                    if not transposed and not accumulate and not scaled:
                        sp = R.from_bits(gb[[0, 8, 9, 11, 13, 14], 0])
                        assert sp.tolist() == [254 * 2.0 ** 120, np.inf, np.inf, -np.inf, 0.0, R.BF16_MAX], what
                        assert gb[13, 0] == 0 and np.isnan(R.from_bits(gb[12])).all(), what


@pytest.mark.parametrize("F", [1, 7, 8, 9, 39, 64, 500, 3703])
def test_spmm_bf16_exact_inputs_bit_for_bit(F):
    check_spmm_bf16(F, True, 100 + F)


@pytest.mark.parametrize("F", [1, 7, 8, 9, 39, 64, 500, 3703])
def test_spmm_bf16_random_inputs_in_bracket(F):
    check_spmm_bf16(F, False, 200 + F)
