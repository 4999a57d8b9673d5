"""tests/dense_ref.py checked without a GPU: fp32 products in several orders stay inside the per-element bounds at
every case shape, the arena sees a write in a guard and in a pad column, a NaN in a pad column never reaches the
reference, and the dispatch restatement agrees with the case tables and with the library's workspace queries.
tests/test_gpu_dense_abi.py holds the kernels of csrc/dense.hip to this reference."""
import numpy as np
import pytest

import dense_ref as R


def _chain(A, B, order):
    """fp32 A [n, K] B [K, J]: rounded products added one k at a time in `order`, every add rounded to fp32"""
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in order:
        acc = acc + A[:, k:k + 1] * B[k:k + 1, :]
    assert acc.dtype == np.float32
    return acc


def _orders(A, B):
    """naive k order, reversed, and four quarter chains that meet in order (the shape of a 4-wave block)"""
    K = A.shape[1]
    yield "naive", _chain(A, B, range(K))
    yield "reversed", _chain(A, B, range(K - 1, -1, -1))
    q = -(-K // 4)
    parts = [_chain(A, B, range(i * q, min((i + 1) * q, K))) for i in range(4)]
    yield "blocked", ((parts[0] + parts[1]) + parts[2]) + parts[3]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "n%d-i%d-o%d" % s)
def test_fp32_products_stay_inside_the_bounds(shape):
    n, f_in, f_out = shape
    M, W, b = R.draw(1, n, f_in), R.draw(2, f_out, f_in), R.draw(3, f_out)
    dY, Ymask = R.draw(4, n, f_out), R.draw_mask(5, n, f_out)
    worst = 0.0
    for act in (R.ACT_IDENTITY, R.ACT_RELU):
        ref, bound = R.linear_fwd(M, W, b, act)
        for name, y in _orders(M, W.T.copy()):
            y = y + b[None, :]
            if act == R.ACT_RELU:
                y = np.maximum(y, np.float32(0))
            ratio, where = R.worst_element(y, ref, bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, ("Y", name, ratio, where)
        refs = R.linear_bwd(dY, Ymask, act, M, W, atb_bf16=0)
        dYm = np.where(Ymask > 0, dY, np.float32(0)) if act == R.ACT_RELU else dY
        for out, A, B in (("dW", dYm.T.copy(), M), ("dM", dYm, W), ("db", dYm.T.copy(), np.ones((n, 1), np.float32))):
            for name, g in _orders(A, B):
                ref, bound = refs[out]
                ratio, where = R.worst_element(g.reshape(ref.shape), ref, bound)
                worst = max(worst, ratio)
                assert ratio <= 1.0, (out, name, ratio, where)
    print(f"n {n} f_in {f_in} f_out {f_out}: largest error / bound {worst:.3f}")
    assert worst > 0.0 or f_in * n == 1         # the bound is compared with a result that does round


def test_a_wrong_product_leaves_the_bound():
    """the bound is tight enough to see one dropped term and a mask taken as Y >= 0"""
    n, f_in, f_out = 33, 39, 16
    M, W, b = R.draw(1, n, f_in), R.draw(2, f_out, f_in), R.draw(3, f_out)
    ref, bound = R.linear_fwd(M, W, b, R.ACT_IDENTITY)
    y = _chain(M[:, :-1], W.T[:-1].copy(), range(f_in - 1)) + b[None, :]
    assert R.worst_element(y, ref, bound)[0] > 1e3
    dY, Ymask = R.draw(4, n, f_out), R.draw_mask(5, n, f_out)
    assert (Ymask == 0).any() and (Ymask < 0).any() and np.signbit(Ymask[Ymask == 0]).any()
    ref, bound = R.linear_bwd(dY, Ymask, R.ACT_RELU, M, W)["db"]
    wrong = np.where(Ymask >= 0, dY, np.float32(0)).astype(np.float64).sum(0)
    assert R.worst_element(wrong, ref, bound)[0] > 1e3
    assert "last row tile" in R.worst_element(np.r_[np.zeros((32, 4)), np.ones((1, 4))], np.zeros((33, 4)), np.ones((33, 4)))[1]


def _arena():
    a = R.Arena()
    a.add("M", 5, 7, R.lead(7, "4"), 1, R.draw(1, 5, 7))
    a.add("W", 3, 7, None, 0, R.draw(2, 3, 7))
    a.add("Y", 5, 3, R.lead(3, "odd"), 1)
    a.add_workspace("ws", 250)
    return a.build()


def test_arena_layout():
    a = _arena()
    assert [a.offset(k) % 4 for k in ("M", "W", "Y", "ws")] == [1, 0, 1, 0]
    assert a.ld("M") == 8 and a.ld("W") == 7 and a.ld("Y") == 5 and R.lead(8, "4") == 12 and R.lead(8, "odd") == 9
    assert np.array_equal(a.get("M"), R.draw(1, 5, 7))
    assert (a.bits("Y") == R.PATTERN).all() and np.isnan(a.get("Y")).all()
    assert a.bits("ws").size == 63 and int(a.inside.sum()) == 35 + 21 + 15 + 63
    assert a.pad["M"].size == 5 and a.pad["Y"].size == 10 and a.pad["W"].size == 0
    for k in ("M", "W", "Y", "ws"):           # GUARD words on both sides of every operand
        lo, hi = a.offset(k), a.offset(k) + a.ops[k]["rows"] * a.ld(k)
        assert not a.inside[lo - R.GUARD:lo].any() and not a.inside[hi:hi + R.GUARD].any()
    assert a.guards_intact() and all(a.pads_intact(k) for k in a.ops)


def test_arena_detects_a_write_in_a_guard():
    for name, at in (("M", -1), ("Y", 5 * 5), ("ws", 63), ("W", -R.GUARD)):
        a = _arena()
        a.host[a.offset(name) + at] = np.float32(0.0).view(np.uint32)
        assert not a.guards_intact(), (name, at)
        assert all(a.pads_intact(k) for k in a.ops)
        assert a.damaged()[0][0] == a.offset(name) + at


def test_arena_detects_a_write_in_a_pad_column():
    a = _arena()
    a.host[a.offset("Y") + 2 * 5 + 3] = np.float32(1.0).view(np.uint32)       # row 2, column 3 of [5, 3] (ld 5)
    assert not a.pads_intact("Y") and a.pads_intact("M") and a.guards_intact()
    a = _arena()
    a.host[a.offset("M") + 4 * 8 + 7] = 0x7FC00000                            # another NaN is still a write
    assert not a.pads_intact("M") and a.pads_intact("Y")


def test_a_nan_in_a_pad_column_does_not_reach_the_reference():
    a = _arena()
    assert np.isnan(a.footprint("M").view(np.float32)).sum() == 5             # the pads are NaN to begin with
    ref, bound = R.linear_fwd(a.get("M"), a.get("W"), None, R.ACT_RELU)
    a.host[a.pad["M"]] = 0xFFC00001
    again, _ = R.linear_fwd(a.get("M"), a.get("W"), None, R.ACT_RELU)
    assert np.isfinite(ref).all() and np.isfinite(bound).all() and np.array_equal(ref, again)
    assert np.array_equal(ref, np.maximum(R.draw(1, 5, 7).astype(np.float64) @ R.draw(2, 3, 7).astype(np.float64).T, 0))


def test_references_on_operands_with_a_known_answer():
    M = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    W = np.array([[1, -1]], np.float32)
    y, bound = R.linear_fwd(M, W, np.array([0.5], np.float32), R.ACT_RELU)
    assert y.tolist() == [[0.0], [0.0], [0.0]] and bound[0, 0] == 6 * R.U24 * 3.5
    y, _ = R.linear_fwd(M, -W, np.array([0.5], np.float32), R.ACT_IDENTITY)
    assert y.tolist() == [[1.5], [1.5], [1.5]]
    dY = np.array([[1], [2], [4]], np.float32)
    Y = np.array([[1], [-0.0], [2]], np.float32)
    g = R.linear_bwd(dY, Y, R.ACT_RELU, M, W)
    assert g["dW"][0].tolist() == [[21.0, 26.0]] and g["db"][0].tolist() == [5.0]
    assert g["dM"][0].tolist() == [[1, -1], [0, 0], [4, -4]]
    g = R.linear_bwd(dY, Y, R.ACT_IDENTITY, M, W, atb_bf16=0)
    assert g["dW"][0].tolist() == [[27.0, 34.0]] and g["db"][1][0] == 7 * R.U24 * 7
    assert R.wgrad_bound(100, 1) == 2 * R.wgrad_bound(100, 0) < R.wgrad_bound(100, 2)


def test_every_kernel_kind_has_a_case_and_the_cases_reach_it():
    """the restated dispatch sends every case to the kernel it was built for, and every value of dense_last_kind is
    some case's"""
    from gae_dgl_amd import _lib
    lib = _lib.load()
    seen = set()
    for c in R.FWD:
        n, K, J = c["n"], c["f_in"], c["f_out"]
        total = lib.gae_linear_fwd_workspace_bytes(n, K, J)
        xw = lib.gae_xw_fwd_workspace_bytes(n, K, J, 0) if 1 <= J <= 32 and K >= 64 else 0
        assert total == max(R.fwd_workspace_bytes_split(n, K, J), xw), c["id"]
        assert not c["ws"] or total > 0, c["id"]
        kind, inst = R.fwd_kind(n, K, J, R.lead(K, c["ld_M"]), not c["mis_M"], not c["mis_W"], total if c["ws"] else 0,
                                xw, c["gemm_rows"], c["linear_wlds"])
        assert kind == c["kind"], (c["id"], kind, inst)
        seen.add((kind, inst))
    for c in R.BWD:
        kind, inst = R.bwd_kind(c)
        assert kind == c["kind"], (c["id"], kind, inst)
        seen.add((kind, inst))
        seen.add(R.wgrad_kind(c))
        assert set(c["want"]) <= {"dW", "db", "dM"} and c["want"]
    assert {k for k, _ in seen} == set(R.KINDS), sorted(set(R.KINDS) - {k for k, _ in seen})
    print(f"{len(R.FWD)} forward and {len(R.BWD)} backward cases reach {len(seen)} kernel instances:")
    for kind, inst in sorted(seen):
        print(f"  {kind:13s} {inst}")
    ids = [c["id"] for c in R.FWD + R.BWD]
    assert len(set(ids)) == len(ids)
    subsets = {frozenset(c["want"]) for c in R.BWD}
    assert len(subsets) == 7                                   # every non-empty subset of {dW, db, dM}
    assert {c["n"] for c in R.FWD} >= {1, 31, 32, 33, 63, 65, 129} and {c["n"] for c in R.BWD} >= {127, 128, 129, 257}
    assert {c["f_in"] for c in R.FWD} >= {1, 3, 7, 32, 33, 39, 64, 128, 130, 192, 520, 2049}
    assert {c["f_out"] for c in R.FWD} >= {1, 7, 16, 32, 33, 130} and {c["f_in"] for c in R.BWD} >= {33, 64, 65, 130}


def test_workspace_plan_matches_the_library():
    """atb_plan restated == gae_linear_bwd_workspace_bytes at the default knob, for every backward shape"""
    from gae_dgl_amd import _lib
    lib = _lib.load()
    for n, f_in, f_out in sorted({(c["n"], c["f_in"], c["f_out"]) for c in R.BWD} | {p[:3] for p in R.PARTIALS}):
        assert lib.gae_linear_bwd_workspace_bytes(n, f_in, f_out) == R.bwd_workspace_bytes(n, f_in, f_out), (n, f_in, f_out)
    assert R.atb_plan(128, 16, 7)[0] == 1 and R.atb_plan(129, 16, 7)[:2] == (2, 128) and R.atb_plan(257, 16, 7)[0] == 3
    assert R.atb_plan(129, 16, 7)[2] == 128 and R.atb_plan(129, 7, 130)[2] == (7 * 130 + 7 + 3) // 4 * 4
