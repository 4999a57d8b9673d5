"""tests/adam_ref.py checked without a GPU: the summation order against float64 and against the orders it must be
told apart from, the fp64 Adam step against torch.optim.Adam in float64, the partial-list layout against its index
formula.  tests/test_gpu_adam_abi.py holds gae_adam_step to this reference."""
import numpy as np
import pytest
import torch

import adam_ref as R

N_CHECK = 257        # elements per list length the conditions on the inputs are asserted on


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_library_order_is_within_the_rounding_bound_of_float64():
    """|sum in library order - float64 sum| <= depth 2^-24 sum |p_q|, depth = the dependent roundings of the order"""
    worst = 0.0
    for q in R.LIST_LENGTHS:
        P = R.wide_partials(q, N_CHECK)
        got = R.sum_in_library_order(P).astype(np.float64)
        exact = P.astype(np.float64).sum(0)
        bound = R.sum_bound(P)
        assert np.all(np.isfinite(got))
        ratio = float((np.abs(got - exact) / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (q, ratio)
    print(f"library order vs float64: largest error / bound = {worst:.3f}")


def test_depth_of_the_order():
    assert [R.sum_depth(q) for q in (1, 32, 33, 64, 65, 128, 129, 1024, 1025)] == [1, 32, 7, 7, 8, 8, 9, 22, 23]


def test_library_order_on_lists_with_a_known_answer():
    """exact small integers: every order gives the same sum; one large partial tells the orders apart by hand"""
    for q in R.LIST_LENGTHS:
        P = np.arange(q * 5, dtype=np.float32).reshape(q, 5) % 7
        assert np.array_equal(R.sum_in_library_order(P), P.astype(np.float64).sum(0).astype(np.float32))
    # 65 partials: lane 0 adds p0 + p64 first.  p0 = 2^24, all others 1: in order, every 1 is lost (2^24 + 1 rounds
    # to even, back to 2^24); in the library's order lane 0 loses p64 the same way and, at off = 32, lane 32's 1; from
    # off = 16 on it meets even integers (2, 4, 8, 16, 32), which 2^24 + even takes exactly: 2^24 + 62.
    P = np.ones((65, 1), np.float32); P[0] = 2.0 ** 24
    assert R.sum_in_library_order(P)[0] == np.float32(2.0 ** 24 + 62)
    inorder = np.float32(0)
    for q in range(65):
        inorder = np.float32(inorder + P[q, 0])
    assert inorder == np.float32(2.0 ** 24)
    # <= 32 partials: plain in-order addition from +0
    P = np.ones((32, 1), np.float32); P[0] = 2.0 ** 24
    assert R.sum_in_library_order(P)[0] == np.float32(2.0 ** 24)
    assert _bits(R.sum_in_library_order(np.full((1, 1), -0.0, np.float32)))[0] == 0        # +0 + -0 = +0


def test_the_inputs_tell_the_orders_apart():
    """conditions on the inputs of the GPU test, asserted so that a later change of inputs cannot make it blind:
    from 33 partials on at least half of the elements differ in bits from plain in-order addition, and from 2 on at
    least 95 % differ from the same list without its last partial"""
    lo_order, lo_last = 1.0, 1.0
    for q in R.LIST_LENGTHS:
        P = R.wide_partials(q, N_CHECK)
        got = _bits(R.sum_in_library_order(P))
        if q >= 33:
            g = np.zeros(N_CHECK, np.float32)
            for k in range(q):
                g = g + P[k]
            share = float((got != _bits(g)).mean())
            lo_order = min(lo_order, share)
            assert share >= 0.5, (q, share)
        if q >= 2:
            share = float((got != _bits(R.sum_in_library_order(P[:-1]))).mean())
            lo_last = min(lo_last, share)
            assert share >= 0.95, (q, share)
    print(f"elements that differ from in-order addition: >= {lo_order:.2f}; from the list without its last partial: "
          f">= {lo_last:.2f}")


def test_every_case_of_the_tables_is_drawn_once():
    for q in R.LIST_LENGTHS:
        for n in R.sizes_for(q):
            P = R.wide_partials(q, n)
            assert P.shape == (q, n) and P.dtype == np.float32
            assert np.array_equal(P, R.wide_partials(q, R.N_DRAW)[:, :n])
    assert sorted(R.LIST_LENGTHS) == R.LIST_LENGTHS and {7, 8, 16, 17, 32, 33, 64, 65, 1024, 1025} <= set(R.LIST_LENGTHS)
    assert len(R.MIXED) == 16 and R.ALL_EMPTY[-1] == (0, 5) and all(n == 0 for n, _ in R.ALL_EMPTY)


@pytest.mark.parametrize("wd", R.WEIGHT_DECAYS)
def test_adam_fp64_matches_torch_in_float64(wd):
    """25 steps against torch.optim.Adam on float64 CPU tensors, both on the fp32-rounded hyper-parameters"""
    lr, b1, b2, eps, wd = R.f32(1e-2), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(wd)
    rng = np.random.default_rng(5)
    p = rng.standard_normal(300)
    m = np.zeros(300); v = np.zeros(300)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for it in range(25):
        g = rng.standard_normal(300) * (1.0 + it)
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, m, v = R.adam_fp64(p, g, m, v, it + 1, lr, b1, b2, eps, wd)
    st = opt.state[tp]
    errs = [R.rel_err(p, tp.detach().numpy()), R.rel_err(m, st["exp_avg"].numpy()), R.rel_err(v, st["exp_avg_sq"].numpy())]
    print(f"adam_fp64 vs torch float64, weight_decay {wd:g}: rel_err {max(errs):.2e}")
    assert max(errs) < 1e-12, errs


def test_the_hyper_parameters_are_the_fp32_values():
    """the reference must step on what the ABI receives: on the Python doubles exp_avg_sq is off by ~1e-5 relative"""
    g = np.ones(4)
    _, _, v32 = R.adam_fp64(np.zeros(4), g, np.zeros(4), np.zeros(4), 1, 0.0, R.f32(0.9), R.f32(0.999), 1e-8, 0.0)
    _, _, v64 = R.adam_fp64(np.zeros(4), g, np.zeros(4), np.zeros(4), 1, 0.0, 0.9, 0.999, 1e-8, 0.0)
    assert 1e-5 < abs(v32[0] - v64[0]) / v64[0] < 2e-5


@pytest.mark.parametrize("kind", R.LAYOUTS)
def test_place_partials_round_trip(kind):
    rng = np.random.default_rng(1)
    for q, n in ((1, 1), (3, 5), (7, 13), (33, 9), (5, 0), (2, 1030)):
        P = rng.standard_normal((q, n)).astype(np.float32)
        stride, row_len, row_pitch = R.layout(kind, n)
        buf = R.place_partials(P, stride, row_len, row_pitch)
        assert buf.dtype == np.float32
        e = np.arange(n)
        for k in range(q):      # the documented formula, element by element
            assert np.array_equal(buf[R.GUARD + k * stride + (e // row_len) * row_pitch + e % row_len], P[k])
        assert int(np.isnan(buf).sum()) == buf.size - q * n
        assert np.isnan(buf[:R.GUARD]).all() and np.isnan(buf[-R.GUARD:]).all() and buf.size >= 2 * R.GUARD
    if kind == "padded_rows":
        assert R.layout(kind, 13) == (3 * 8 + 24, 5, 8)
    with pytest.raises(AssertionError):
        R.place_partials(np.zeros((2, 8), np.float32), 4, 8, 8)        # partials that overlap
