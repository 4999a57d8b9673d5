"""tests/loss_pieces_ref.py: the piece rounding of the symmetric fused loss kernel, modelled in numpy, on the very
inputs tests/test_gpu_loss_range.py gives the kernel.  Shows that the suite's gradient bound is attainable from the
inputs alone, and that the fp16 form holds it on every input the range guard leaves on that form -- because only
P V = (sigmoid(S) - 1/2) Zt runs on the pieces."""
import numpy as np
import pytest

import loss_pieces_ref as R


@pytest.fixture(scope="module", params=R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def problem(request):
    n, d = request.param
    src, dst = R.sym_edges(n, seed=n)
    pr, exact = R.Problem(n, src, dst), {}

    def ref(name, Z, mask):                 # the fp64 reference of an input, computed once for the tests of a shape
        if name not in exact:
            exact[name] = pr.exact(Z, mask)
        return exact[name]
    return n, d, pr, ref


def _cases(n, d, in_range_only):
    ins = R.in_range_inputs(n, d)
    for name, Z in ins.items():
        yield name, Z, None
        if name.startswith("ladder"):
            yield name + "+mask", Z, R.given_mask(n, d)
    if not in_range_only:
        for name, Z in R.out_of_range_inputs(n, d).items():
            yield name, Z, None


def test_pieces_sum_to_the_value():
    v = (np.random.default_rng(0).standard_normal(4000) * np.logspace(-9, 4.5, 4000)).astype(np.float32)
    f, b3, a = R.f16_pieces(v), R.bf16_pieces(v, 3), np.abs(v.astype(np.float64))
    assert np.all(np.abs(b3 - v) <= 2.0 ** -24 * a)                               # three bf16 pieces: the fp32 value
    # two fp16 pieces: 22 bits only while the SECOND piece is a normal fp16 number, i.e. from |v| = 2^-3 upwards; below
    # that the remainder v - hi is an fp16 subnormal (spacing 2^-24) and the error an absolute 2^-25
    assert np.all(np.abs(f - v) <= np.maximum(2.0 ** -22 * a, 2.0 ** -25))
    mid = (a >= 2.0 ** -14) & (a < 2.0 ** -4)
    assert np.any(np.abs(f - v)[mid] > 2.0 ** -22 * a[mid])                       # (not 22 bits from 2^-14 on)
    assert np.all(R.f16_pieces(np.float32([1e-8, -2e-8])) == 0.0)                 # ... of the whole value in the end
    assert not np.isfinite(R.f16_pieces(np.float32([65520.0]))[0]) and R.f16_pieces(np.float32([65504.0]))[0] == 65504.0


def test_three_bf16_pieces_meet_the_bounds_on_every_input(problem):
    """the bound is attainable: the kernel's three-piece bf16 form (three pieces for S, two for P and V, the 1/2 and
    edge parts exact) on every finite input of the GPU file, those beyond the fp16 guard included"""
    n, d, pr, ref = problem
    for name, Z, mask in _cases(n, d, in_range_only=False):
        le, ge = R.errors(pr.model(Z, mask, "bf16"), ref(name, Z, mask))
        assert le <= R.TOL and ge < R.GRAD_BOUND, (name, le, ge)


def test_fp16_pieces_meet_the_bounds_on_every_input_kept_on_them(problem):
    """the kernel keeps every call with max |Zt| <= 32768 on the fp16 form, whatever its smallest values are: in the
    kernel's arrangement the model holds the gradient bound on all of them with more than 2x headroom"""
    n, d, pr, ref = problem
    worst = 0.0
    for name, Z, mask in _cases(n, d, in_range_only=True):
        assert float(np.abs(Z).max()) <= R.F16_MAX
        le, ge = R.errors(pr.model(Z, mask, "f16"), ref(name, Z, mask))
        assert le <= R.TOL and ge < R.GRAD_BOUND, (name, le, ge)
        worst = max(worst, ge)
    assert worst < R.GRAD_BOUND / 2


def test_rounded_values_against_the_whole_gradient_would_not():
    """why the arrangement matters: were the rounded Zt multiplied with all of G (its 1/2 and edge parts included),
    every value's 2^-25 / |z| would reach the gradient -- the fp16 pieces would miss the bound from a scale of 1e-4
    downwards and lose the gradient altogether at 1e-8, where three bf16 pieces still hold it"""
    n, d = R.SHAPES[0]
    src, dst = R.sym_edges(n, seed=n)
    pr = R.Problem(n, src, dst)
    got = {}
    for s in (1.0, 1e-2, 1e-4, 1e-6, 1e-8):
        Z = R.ladder_input(n, d, s)
        ref = pr.exact(Z)
        got[s] = R.errors(pr.model(Z, None, "f16", centred=False), ref)[1]
        assert R.errors(pr.model(Z, None, "bf16x3", centred=False), ref)[1] < 1e-7
    assert got[1.0] < 1e-6 and got[1e-2] < R.GRAD_BOUND
    assert got[1e-4] > R.GRAD_BOUND and got[1e-6] > 100 * R.GRAD_BOUND and got[1e-8] > 0.5
