"""gae_dropout_mask and gae_normal_noise through the raw C ABI against tests/noise_ref.py: the dropout multipliers bit
for bit, the noise inside NOISE_A rad + NOISE_B |z| of float64 Box-Muller on the same fp32 uniforms (an error in the
counter layout, the word-to-uniform map or the sin / cos lanes moves values by O(1); the bound is 1e-6-sized), outputs
between canaries, and the noise gae_x_vgae_head_prep draws inside its launch equal to gae_normal_noise's bit for bit.
Sizes: one block of four and its tails, 1023 / 1025 around a thread block's 1024 elements, and 2 097 157 = one
grid-stride trip past the 2048 x 256 x 4 elements a launch covers at once."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import noise_ref as R
import vgae_abi as A

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 3, 4, 5, 1023, 1025, 2 * 1024 * 1024 + 5]
PS = [0.0, 0.1, 0.25, 0.5, 0.999]
OFFSETS = [0, 512, (1 << 32) + 3]
DRAWS = [None, 5, (1 << 32) + 5, (1 << 63) + 1]


def combos(n):
    """every (offset, draw) for the short sizes; for the long one a set that still holds every offset and every draw"""
    if n < 100000:
        return list(itertools.product(OFFSETS, DRAWS))
    return [(OFFSETS[i % 3], DRAWS[i % 4]) for i in range(4)]


def call_dropout(n, p, offset, draw):
    out, dd = A.Canaried(n), A.draw_tensor(draw)
    with torch.cuda.device(A.DEV):
        rc = A.lib().gae_dropout_mask(out.ptr(), n, p, A.SEED, offset, A.ptr(dd), A.stream())
    assert rc == 0, (rc, A.lib().gae_last_error())
    return out.read()


def call_noise(n, offset, draw, seed=A.SEED):
    out, dd = A.Canaried(n), A.draw_tensor(draw)
    with torch.cuda.device(A.DEV):
        rc = A.lib().gae_normal_noise(out.ptr(), n, seed, offset, A.ptr(dd), A.stream())
    assert rc == 0, (rc, A.lib().gae_last_error())
    return out.read()


@pytest.mark.parametrize("n", SIZES)
def test_dropout_mask_equals_the_restatement_bit_for_bit(n):
    for offset, draw in combos(n):
        words = R.philox_words(R._counters(n, offset), (draw or 0) & R.M32, (draw or 0) >> 32, A.SEED).reshape(-1)[:n]
        for p in PS:
            got, intact = call_dropout(n, p, offset, draw)
            ref = R.dropout_of_words(words, p)
            bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
            assert bad.size == 0, (n, p, offset, draw, bad[:8].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())
            assert intact, (n, p, offset, draw, "written outside [0, n_elems)")


@pytest.mark.parametrize("p,block,lane", [(0.5, 1929882, 3), (0.25, 4590299, 1)])
def test_dropout_keeps_a_draw_equal_to_p(p, block, lane):
    """block `block` of draw 0 holds u == p exactly in element `lane` (found by searching the restated stream; asserted
    on the host first): the contract is u >= p, so that element is kept"""
    words = R.philox_words([block], 0, 0, A.SEED)[0]
    assert int(words[lane]) >> 8 == int(p * (1 << 24))
    got, intact = call_dropout(4, p, block, None)
    ref = R.dropout_mask(4, p, A.SEED, block, 0)
    assert ref[lane] == np.float32(1) / (np.float32(1) - np.float32(p))
    assert intact and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (got.tolist(), ref.tolist())


@pytest.mark.parametrize("n", SIZES)
def test_normal_noise_is_box_muller_on_the_restated_uniforms(n):
    worst, measured = 0.0, 0.0
    for offset, draw in combos(n):
        got, intact = call_noise(n, offset, draw)
        u1, u2 = R.normal_uniforms(n, A.SEED, offset, draw or 0)
        ref, rad = R.box_muller(u1, u2, (np.arange(n) & 1) == 1)              # = R.normal_noise, keeping rad and u1
        bound = R.NOISE_A * rad + R.NOISE_B * np.abs(ref)
        ratio, at = R.worst(got, ref, bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(rad > 0, np.abs(got - ref) / (rad + np.abs(ref)), 0.0).max()
        worst, measured = max(worst, ratio), max(measured, float(m))
        assert ratio <= 1.0, (n, offset, draw, ratio, at, float(got[at]), float(ref[at]), float(bound[at]))
        assert intact, (n, offset, draw, "written outside [0, n_elems)")
        assert np.all(got[u1 == 1.0] == 0.0)                  # rad = 0: an exact zero (bound 0 admits nothing else)
        # the dropout stream of the same draw, pushed through the same Box-Muller, is another sequence
        dd = (draw or 0)
        wd = R.philox_words(R._counters(n, offset), dd & R.M32, dd >> 32, A.SEED)
        other = R.box_muller(np.repeat(R.u1_of_words(wd[:, 0::2]).reshape(-1), 2)[:n],
                             np.repeat(R.u2_of_words(wd[:, 1::2]).reshape(-1), 2)[:n], (np.arange(n) & 1) == 1)[0]
        assert np.abs(got - other).max() > 1e-3, (n, offset, draw, "the noise reads the dropout stream")
    print(f"NOISE n={n}: largest error / bound {worst:.3f}, largest |gpu - ref| / (rad + |z|) {measured:.3e}")


def test_normal_noise_seed_halves_and_determinism():
    """both halves of the seed key the stream, and a second call gives the same bits"""
    n = 1025
    base = call_noise(n, 7, 3)[0]
    assert np.array_equal(base.view(np.uint32), call_noise(n, 7, 3)[0].view(np.uint32))
    for seed in (A.SEED ^ 1, A.SEED ^ (1 << 32), A.SEED ^ (1 << 63)):
        got = call_noise(n, 7, 3, seed)[0]
        ref, bound = R.normal_noise(n, seed, 7, 3)
        assert R.worst(got, ref, bound)[0] <= 1.0 and not np.array_equal(got, base)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_noise_drawn_inside_the_head_launch_is_the_same_stream(n):
    offset, draw = 7, (1 << 32) + 1
    rng = np.random.default_rng(n)
    mu, ls = (rng.standard_normal((n, 16)).astype(np.float32) for _ in range(2))
    a = A.arena()
    a.add("mu", n, 16, 16, 0, mu).add("ls", n, 16, 16, 0, ls).add("eps", n, 16).add("z", n, 16)
    a.add_workspace("klp", 8 * ((n + 63) // 64))
    d = A.Device(a.build())
    w, dd, blocks = A.PrepWorkspace(n), A.draw_tensor(draw), ctypes.c_int64(0)
    with torch.cuda.device(A.DEV):
        rc = A.lib().gae_x_vgae_head_prep(d.ptr("mu"), d.ptr("ls"), 16, d.ptr("eps"), 1, A.SEED, offset, A.ptr(dd), n, 16,
                                          d.ptr("z"), ctypes.byref(w.lay), d.ptr("klp"), (n + 63) // 64,
                                          ctypes.byref(blocks), A.stream())
    assert rc == 0, (rc, A.lib().gae_last_error())
    d.download()
    d.check_memory(f"n={n}", ["mu", "ls"], ["eps", "z"])
    eps = d.a.get("eps").reshape(-1)
    alone, intact = call_noise(n * 16, offset, draw)
    assert intact and np.array_equal(eps.view(np.uint32), alone.view(np.uint32))
    ref, bound = R.normal_noise(n * 16, A.SEED, offset, draw)
    ratio, at = R.worst(eps, ref, bound)
    print(f"NOISE in-launch n={n}: largest error / bound {ratio:.3f}")
    assert ratio <= 1.0, (n, ratio, at)
