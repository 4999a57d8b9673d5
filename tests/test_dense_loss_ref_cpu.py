"""tests/dense_loss_ref.py checked without a GPU: fp32 restatements of the decoder products (several summation orders)
and of the BCE element stay inside the per-element bounds; each planted error leaves its bound -- among them the
gradient with every y = 0 entry zeroed, which the norm-wise measure of test_bce_logits_kernel accepts; the restated
dispatch sends every case to the kind its id names; the restated workspace sizes are the library's.
tests/test_gpu_dense_loss_abi.py holds the kernels to this reference."""
import numpy as np
import pytest

import dense_loss_ref as L
import dense_ref as R
from test_dense_ref_cpu import _orders


# ---------------------------------------------------------------------------------------------- the reference alone
@pytest.mark.parametrize("shape", L.DECODER_SHAPES, ids=lambda s: "n%d-d%d" % s)
def test_fp32_decoder_products_stay_inside_the_bounds(shape):
    n, d = shape
    Z, mask, G = L.decoder_inputs(n, d)
    worst = 0.0
    for m in (None, mask):
        zt = L.masked_z(Z, m)
        ref, bound = L.decoder_dense(Z, m)
        for name, out in _orders(zt, zt.T.copy()):
            ratio, where = R.worst_element(out, ref, bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, ("out", name, ratio, where)
        ref, bound = L.decoder_dense_bwd(G, Z, m, 0)         # the exact-fp32 bound is the tightest of the three
        for (n1, t1), (n2, t2) in zip(_orders(G, zt), list(_orders(G.T.copy(), zt))[::-1]):
            dZ = t1 + t2
            if m is not None:
                dZ = dZ * m
            assert dZ.dtype == np.float32
            ratio, where = R.worst_element(dZ, ref, bound)
            worst = max(worst, ratio)
            assert ratio <= 1.0, ("dZ", n1, n2, ratio, where)
    print(f"n {n} d {d}: largest error / bound {worst:.3f}")
    assert worst > 0.0


def _bce_fp32(x, y, pw, sigmoid_swapped=False):
    """bce_elem restated with numpy's fp32 exp and log1p: (loss, grad), every operation rounded to fp32, the terms
    added in float64 as the kernel does"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    one = np.float32(1)
    lw = one + (np.float32(pw) - one) * y
    with np.errstate(under="ignore"):
        e = np.exp(-np.abs(x))
        sp = np.maximum(-x, np.float32(0)) + np.log1p(e)
        pos = (x < 0) if sigmoid_swapped else (x >= 0)
        sn = np.where(pos, e / (one + e), one / (one + e))
        l = (one - y) * x + lw * sp
        g = ((one - y) - lw * sn) * np.float32(1.0 / x.size)
    assert e.dtype == sp.dtype == sn.dtype == l.dtype == g.dtype == np.float32
    return np.float32(l.astype(np.float64).sum() * (1.0 / x.size)), g


def _bce_ratios(x, y, pw, loss, g):
    ref = L.bce_logits(x, y, pw)
    return abs(float(loss) - ref["loss"]) / ref["loss_bound"], R.worst_element(g, ref["grad"], ref["grad_bound"])[0]


def test_fp32_bce_stays_inside_the_bounds():
    """numpy's fp32 exp is not the kernel's __expf, but it is an fp32 restatement of every other operation: at most
    half of either bound on the value ladder and on the random cases"""
    worst = [0.0, 0.0]
    for c in L.BCE:
        if c["rows"] * c["cols"] > 301 * 517:
            continue
        x, y = L.bce_inputs(c)
        rl, rg = _bce_ratios(x, y, c["pw"], *_bce_fp32(x, y, c["pw"]))
        worst = [max(worst[0], rl), max(worst[1], rg)]
        assert rl <= 0.5 and rg <= 0.5, (c["id"], rl, rg)
    print(f"fp32 numpy BCE: largest loss error / bound {worst[0]:.3f}, gradient {worst[1]:.3f}")
    assert worst[1] > 0.0


def test_bce_bounds_are_finite_and_cover_the_ladder():
    ladder = [c for c in L.BCE if c["ladder"]]
    assert {c["pw"] for c in ladder} == set(L.POS_WEIGHTS)
    x, y = L.bce_inputs(ladder[0])
    assert x.shape == (3, 22) and {float(v) for v in np.abs(x[0])} == {float(np.float32(v)) for v in L.LADDER}
    assert (np.signbit(x[0]).sum(), sorted(set(y.reshape(-1).tolist()))) == (11, [0.0, 1.0, 2.0])
    for c in ladder:
        ref = L.bce_logits(x, y, c["pw"])
        for k in ("grad", "grad_bound", "terms", "term_bound"):
            assert np.isfinite(ref[k]).all() and ref[k].shape == x.shape, (c["id"], k)
        assert (ref["grad_bound"] > 0).all() or c["pw"] == 0.5
        assert np.isfinite(ref["loss"]) and ref["loss_bound"] > 0


# ---------------------------------------------------------------------------------------------- planted errors
def test_planted_decoder_errors_leave_their_bounds():
    n, d = 129, 39
    Z, mask, G = L.decoder_inputs(n, d)
    zt = L.masked_z(Z, mask).astype(np.float64)
    ref, bound = L.decoder_dense(Z, mask)
    one_side = zt @ Z.astype(np.float64).T                      # the mask on A only
    assert R.worst_element(one_side, ref, bound)[0] > 1e3
    assert R.worst_element(zt @ zt.T, ref, bound)[0] == 0.0
    ref, bound = L.decoder_dense_bwd(G, Z, mask, 2)              # the widest of the three bounds
    G64, m64 = G.astype(np.float64), mask.astype(np.float64)
    assert R.worst_element((G64 @ zt) * m64, ref, bound)[0] > 1e3                       # no transpose term
    assert R.worst_element((G64 @ zt) * 2 * m64, ref, bound)[0] > 1e3                   # G taken as symmetric
    assert R.worst_element(G64 @ zt + G64.T @ zt, ref, bound)[0] > 1e3                  # no final mask
    assert R.worst_element((G64 @ zt + G64.T @ zt) * m64, ref, bound)[0] == 0.0
    # without a mask the same three
    ref, bound = L.decoder_dense_bwd(G, Z, None, 2)
    assert R.worst_element(G64 @ Z.astype(np.float64), ref, bound)[0] > 1e3


def test_planted_bce_errors_leave_their_bounds():
    x, y, pw = L.parity_bce_inputs()
    ref = L.bce_logits(x, y, pw)
    loss, g = _bce_fp32(x, y, pw)
    assert max(_bce_ratios(x, y, pw, loss, g)) <= 0.5
    # sigmoid(-x) with its branches swapped at x = 0: sigmoid(+x)
    loss_s, g_s = _bce_fp32(x, y, pw, sigmoid_swapped=True)
    assert _bce_ratios(x, y, pw, loss_s, g_s)[1] > 1e3
    # y = 2 (a duplicate edge) treated as y = 1
    assert (y == 2).any()
    loss_c, g_c = _bce_fp32(x, np.minimum(y, 1), pw)
    rl, rg = _bce_ratios(x, y, pw, loss_c, g_c)
    assert rl > 1e3 and rg > 1e3
    # 2 % too large everywhere
    assert _bce_ratios(x, y, pw, loss, g * np.float32(1.02))[1] > 1e3


def test_the_norm_wise_measure_accepts_a_gradient_without_its_negatives():
    """the gap this reference closes: on the inputs of test_gpu_parity.py::test_bce_logits_kernel a gradient with every
    y = 0 entry (98 % of the matrix) set to zero, and one that is 2 % too large everywhere, both score below that
    test's 1e-5 -- max|ref| is 4.8e-4, so its max(1, max|ref|) makes the bound an absolute 1e-5 -- and both leave the
    per-element bound by orders of magnitude"""
    x, y, pw = L.parity_bce_inputs()
    ref = L.bce_logits(x, y, pw)
    assert np.abs(ref["grad"]).max() < 4.9e-4 and 0.98 < (y == 0).mean() < 0.981
    zeroed = np.where(y == 0, 0.0, ref["grad"])
    scaled = 1.02 * ref["grad"]
    old = L.old_rel_err(zeroed, ref["grad"]), L.old_rel_err(scaled, ref["grad"])
    new = [R.worst_element(g, ref["grad"], ref["grad_bound"])[0] for g in (zeroed, scaled)]
    print(f"zeroed y = 0 entries: old measure {old[0]:.3g}, error / bound {new[0]:.3g}; "
          f"2 % too large: old measure {old[1]:.3g}, error / bound {new[1]:.3g}")
    assert old[0] < 1e-5 and old[1] < 1e-5
    assert abs(old[0] - 6.43e-6) < 1e-7 and abs(old[1] - 9.64e-6) < 1e-7
    assert new[0] > 1e3 and new[1] > 1e3


# ---------------------------------------------------------------------------------------------- dispatch and sizes
def test_every_decoder_case_reaches_the_kind_its_id_names():
    seen = set()
    for c in L.FWD:
        kind, inst = L.fwd_kind(c)
        assert kind == c["kind"] == "tiled", c["id"]
        seen.add((kind, inst))
    term1 = set()
    for c in L.BWD:
        for mask in (0, 1):
            kind, inst, t1 = L.bwd_kind(c, mask)
            assert kind == c["kind"] and c["id"].startswith(kind[4:] + "-"), (c["id"], kind, inst)
            seen.add((kind, inst))
            term1.add(t1)
    assert {k for k, _ in seen} == {"tiled", "atb_bf16", "atb_narrow", "atb_vec", "atb_scalar"}
    assert {i for k, i in seen if k == "atb_bf16"} == {"atb_bf16_kernel<p3=1>", "atb_bf16_kernel<p3=0>"}
    assert {i for k, i in seen if k == "tiled"} == {f"gemm_kernel<4, bt=1, pro={p}, mask_b={b}, vec_a={v}>"
                                                     for p, b in (("mul_mask", 1), ("none", 0)) for v in (0, 1)}
    for nt in (1, 2, 4):          # term 1 with a mask: every width of the masked tiled kernel, vector and scalar rows of G
        assert {f"gemm_kernel<{nt}, bt=0, mask_b=1, vec_a={v}>" for v in (0, 1)} <= term1, nt
    assert any(t.startswith("stream:") for t in term1) and any(t.startswith("tiled:") for t in term1)
    print(f"{len(L.FWD)} forward and {len(L.BWD)} x 2 backward cases; term 1 of the backward runs:")
    for t in sorted(term1):
        print("  ", t)
    ids = [c["id"] for c in L.FWD + L.BWD + L.BCE + L.CSR]
    assert len(set(ids)) == len(ids)
    assert {c["n"] for c in L.FWD} == {1, 31, 128, 129, 257} and {c["d"] for c in L.FWD} == {1, 3, 16, 32, 33, 39, 65, 130}
    assert {c[k] for c in L.FWD for k in ("ld_Z", "ld_out")} == {"w", "4", "odd"}
    assert {c["ld_dZ"] for c in L.BWD} == {"w", "4", "odd"}
    # the column tail of atb_bf16_kernel needs ldg > n; the three-slot plan needs n > 256
    assert any(c["kind"] == "atb_bf16" and L.ld_of(c["n"], c["ld_G"]) > c["n"] and c["n"] % 4 for c in L.BWD)
    assert R.atb_plan(257, 32, 257)[0] == 3 and R.atb_plan(132, 16, 132)[0] == 2
    # a contiguous G: 132 nodes take the bf16 kernel, 129 the scalar one
    by = {(c["n"], c["d"], c["ld_G"], c["atb_bf16"]): c["kind"] for c in L.BWD}
    assert by[(132, 16, "w", 1)] == "atb_bf16" and by[(129, 16, "w", 1)] == "atb_scalar"


def test_bce_and_csr_case_tables():
    shapes = {(c["rows"], c["cols"]) for c in L.BCE if not c["ladder"]}
    assert shapes == {(1, 1), (1, 255), (16, 16), (1, 257), (257, 1), (301, 517), (733, 719)}
    assert 733 * 719 > L.BCE_GRID_ELEMS and (733 * 719 - L.BCE_GRID_ELEMS) % 256
    assert {c["mode"] for c in L.BCE} == {"grad", "null", "alias"} and {c["pw"] for c in L.BCE} == set(L.POS_WEIGHTS)
    for c in L.BCE:
        if c["mode"] == "grad":       # three different leading dimensions wherever pad columns can differ
            lds = [R.lead(c["cols"], c[k]) for k in ("ld_x", "ld_y", "ld_g")]
            assert len(set(lds)) == 3 or c["cols"] == 1 and c["rows"] == 1, c["id"]
    big = [c for c in L.CSR if c["id"] == "1x130-ld131-row-of-200"][0]
    assert big["indptr"].tolist() == [0, 200]
    assert any(c["indices"].size == 0 for c in L.CSR) and any(c["ld"] > c["n_cols"] for c in L.CSR)
    assert {(c["n_rows"], c["n_cols"]) for c in L.CSR} == {(5, 9), (130, 1), (1, 130)}
    for c in L.CSR:
        ref = L.csr_to_dense(c["indptr"], c["indices"], c["n_rows"], c["n_cols"])
        assert ref.sum() == c["indices"].size and ref.shape == (c["n_rows"], c["n_cols"])
    assert max(L.csr_to_dense(c["indptr"], c["indices"], c["n_rows"], c["n_cols"]).max() for c in L.CSR) == 70
    assert (np.diff([c for c in L.CSR if c["id"] == "5x9-ld9-empty-rows"][0]["indptr"]) == 0).sum() == 3


def test_workspace_sizes_match_the_library(tuning):
    from gae_dgl_amd import _lib
    lib = _lib.load()
    assert lib.gae_bce_logits_workspace_bytes() == L.BCE_WORKSPACE_BYTES
    for knob in (1, 0, 2):
        tuning("atb_bf16", knob)
        for n, d in L.DECODER_SHAPES:
            assert lib.gae_decoder_dense_bwd_workspace_bytes(n, d) == L.bwd_workspace_bytes(n, d, knob), (knob, n, d)
    assert lib.gae_decoder_dense_bwd_workspace_bytes(-1, 4) < 0


# ---------------------------------------------------------------------------------------------- known answers
def test_references_on_operands_with_a_known_answer():
    Z = np.array([[1, 2], [3, 4], [5, 6]], np.float32)
    m = np.array([[1, 0], [1, 1], [0, 2]], np.float32)
    out, bound = L.decoder_dense(Z, m)
    assert out.tolist() == [[1, 3, 0], [3, 25, 48], [0, 48, 144]] and bound[1, 2] == 6 * R.U24 * 48
    G = np.array([[1, 2, 0], [0, 1, 0], [4, 0, 1]], np.float32)
    dZ, bound = L.decoder_dense_bwd(G, Z, None)
    assert dZ.tolist() == (G.astype(np.float64) @ Z + G.T.astype(np.float64) @ Z).tolist()
    dZ, bound = L.decoder_dense_bwd(G, Z, m)
    zt = (Z * m).astype(np.float64)
    assert dZ.tolist() == ((G @ zt + G.T @ zt) * m).tolist() and (bound[m == 0] == 0).all() and (bound[m != 0] > 0).all()
    r = L.bce_logits(np.zeros((1, 3), np.float32), np.array([[0, 1, 2]], np.float32), 0.5)
    ln2 = np.log(2.0)
    assert np.allclose(r["terms"], [[ln2, 0.5 * ln2, 0.0]], rtol=0, atol=1e-15)        # lw = 1, 0.5, 0
    assert np.allclose(r["grad"] * 3, [[0.5, -0.25, -1.0]], rtol=0, atol=1e-15)
    r = L.bce_logits(np.array([[1e4, -1e4]], np.float32), np.array([[1, 1]], np.float32), 1023.0)
    assert r["terms"].tolist() == [[0.0, 1023e4]] and r["grad"].tolist() == [[0.0, -1023 / 2]]
    assert L.csr_to_dense(np.array([0, 3, 3]), np.array([1, 1, 0]), 2, 2).tolist() == [[1, 2], [0, 0]]
    n, d = L.CHAIN[0][:2]
    Z, mask, src, dst = L.chain_inputs(n, d)
    loss, dZ, pw, A = L.chain_ref(Z, mask, src, dst)
    assert A.sum() == src.size and A.max() >= 2 and pw == (n * n - src.size) / src.size
    assert np.isfinite(loss) and dZ.shape == (n, d) and 0 < np.abs(dZ).max() < 1
