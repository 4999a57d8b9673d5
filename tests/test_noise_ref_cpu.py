"""tests/noise_ref.py is itself checked: its Philox against the scalar restatement of tests/sampled_ref.py and the
published Random123 known answers, the fp32 corners of u1, the distribution of the restated noise (Kolmogorov-Smirnov
and correlations inside and across blocks of four -- once tests/test_gpu_noise.py ties the kernel to the restatement
this is the distribution test of the kernel), the dropout rule (keep-rate, `>=` not `>`), and the head formulas against
torch fp64 autograd.  Then the argument checks of gae_vgae_head_fwd / gae_vgae_head_bwd / gae_x_vgae_head_prep through
ctypes with fake pointers: every refusal comes back before any launch and gae_last_error() names the quantity."""
import ctypes

import numpy as np
import pytest
import torch

import noise_ref as R
import sampled_ref

GAE_OK, E_NULL, E_SIZE, E_ALIGN, E_WORKSPACE, E_RANGE = 0, -1, -2, -3, -5, -6
FAKE = 0x10000          # a 16-byte aligned non-NULL "device pointer": the checks must return before it is dereferenced
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ Philox
def test_philox_known_answers():
    zero = R.philox_words([0], 0, 0, 0)[0]
    assert [f"{int(w):08x}" for w in zero] == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    ones = R.philox_words([M64], 0xFFFFFFFF, 0xFFFFFFFF, M64)[0]
    assert [f"{int(w):08x}" for w in ones] == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert sampled_ref.philox4x32_10(0, 0, 0) == [int(w) for w in zero]
    assert sampled_ref.philox4x32_10(M64, M64, M64) == [int(w) for w in ones]


def test_philox_words_equal_the_scalar_function():
    rng = np.random.default_rng(0)
    trip = [(int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 1 << 63)) * 2 + 1,
             int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))) for _ in range(64)]
    for ctr, draw, seed in trip:
        got = R.philox_words(np.array([ctr, (ctr + 1) & M64], np.uint64), draw & R.M32, draw >> 32, seed)
        assert [int(w) for w in got[0]] == sampled_ref.philox4x32_10(ctr, draw, seed)
        assert [int(w) for w in got[1]] == sampled_ref.philox4x32_10((ctr + 1) & M64, draw, seed)


def test_counter_layouts():
    """dropout: draw low in word 2, high in word 3; noise: tag ^ draw high in word 2, draw low in word 3; the block
    counter is offset + q modulo 2^64"""
    seed, draw, off = 0x1234567890ABCDEF, (7 << 32) + 5, M64 - 1
    m = R.dropout_mask(12, 0.5, seed, off, draw)
    e1, e2 = R.normal_uniforms(12, seed, off, draw)
    for q in range(3):
        ctr = (off + q) & M64
        wd = np.array(sampled_ref.philox4x32_10(ctr, draw, seed), np.uint32)
        assert np.array_equal(m[4 * q:4 * q + 4], R.dropout_of_words(wd, 0.5))
        wn = np.array(sampled_ref.philox4x32_10(ctr, (R.NOISE_TAG ^ 7) | (5 << 32), seed), np.uint32)
        assert np.array_equal(e1[4 * q:4 * q + 4], np.repeat(R.u1_of_words(wn[0::2]), 2))
        assert np.array_equal(e2[4 * q:4 * q + 4], np.repeat(R.u2_of_words(wn[1::2]), 2))
    # a shorter tensor is a prefix; an offset shifts by whole blocks
    assert np.array_equal(R.dropout_mask(5, 0.5, seed, off, draw), m[:5])
    assert np.array_equal(R.dropout_mask(8, 0.5, seed, (off + 1) & M64, draw), m[4:12])
    z, _ = R.normal_noise(12, seed, off, draw)
    assert np.array_equal(R.normal_noise(7, seed, off, draw)[0], z[:7])
    assert np.array_equal(R.normal_noise(8, seed, (off + 1) & M64, draw)[0], z[4:12])


# ------------------------------------------------------------------------------------------------ noise
def test_u1_corners():
    w = np.array([0, 0x7FFFFF00, 0x80000100, 0xFFFFFF00], np.uint32)
    u1 = R.u1_of_words(w)
    assert u1.dtype == np.float32
    assert u1.astype(np.float64).tolist() == [2.0 ** -25, 8388607.5 * 2.0 ** -24, 8388610.0 * 2.0 ** -24, 1.0]
    z, rad = R.box_muller(u1, R.u2_of_words(np.array([0x12345600] * 4, np.uint32)), np.array([0, 1, 0, 1], bool))
    assert rad[3] == 0.0 and z[3] == 0.0
    assert R.box_muller(u1[3:], R.u2_of_words(w[1:2]), np.array([False]))[0][0] == 0.0       # both members of the pair
    assert abs(rad[0] - np.sqrt(50.0 * np.log(2.0))) < 1e-12 and rad.max() < 5.9
    assert float(R.u2_of_words(w).max()) < 1.0 and float(R.u2_of_words(w).min()) == 0.0


@pytest.fixture(scope="module", params=[3, 7, 12345])
def noise(request):
    z, bound = R.normal_noise(1 << 20, request.param, 0, 0)
    return request.param, z, bound


def test_noise_is_standard_normal(noise):
    from scipy import stats
    seed, z, bound = noise
    N = z.size
    D = stats.kstest(z, "norm").statistic
    print(f"seed {seed}: sqrt(N) D = {np.sqrt(N) * D:.3f}, max |z| = {np.abs(z).max():.3f}")
    assert np.sqrt(N) * D < 1.63                                  # the 1 % point of the Kolmogorov distribution
    assert np.abs(z).max() < 5.9                                  # u1 >= 2^-25
    assert (bound >= 0).all() and bound.max() < (R.NOISE_A + R.NOISE_B) * 5.9 < 1e-4     # a layout error moves values by O(1)


def test_noise_has_no_correlation_inside_or_across_blocks(noise):
    seed, z, _ = noise
    q = z.reshape(-1, 4)

    def score(a, b):
        return abs(np.corrcoef(a, b)[0, 1]) * np.sqrt(a.size)
    pairs = {"(0,1)": score(q[:, 0], q[:, 1]), "(2,3)": score(q[:, 2], q[:, 3]), "(0,2)": score(q[:, 0], q[:, 2]),
             "(1,3)": score(q[:, 1], q[:, 3]), "lag 4": score(z[:-4], z[4:])}
    print(f"seed {seed}: |r| sqrt(n) " + ", ".join(f"{k} {v:.2f}" for k, v in pairs.items()))
    assert max(pairs.values()) < 4.0
    # the squares of a pair: independent for Box-Muller on two independent uniforms, correlated for a shared one
    sq = score(q[:, 0] ** 2, q[:, 1] ** 2)
    print(f"seed {seed}: squares of a pair {sq:.2f}")
    assert sq < 4.0


# ------------------------------------------------------------------------------------------------ dropout
def test_dropout_keep_rate():
    n, p = 1 << 20, 0.1
    m = R.dropout_mask(n, p, 3, 0, 0)
    assert set(np.unique(m).tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    kept = int((m != 0).sum())
    zscore = abs(kept - n * (1 - p)) / np.sqrt(n * p * (1 - p))
    print(f"keep-rate z-score {zscore:.2f}")
    assert zscore < 4.0


@pytest.mark.parametrize("p", [0.25, 0.5])
def test_dropout_drops_exactly_p_of_the_u_grid(p):
    """u takes the 2^24 values k 2^-24; p 2^24 is an integer, so exactly that many are < p: `>=` keeps u == p"""
    words = np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)
    m = R.dropout_of_words(words, p)
    assert int((m == 0).sum()) == int(p * (1 << 24))
    at_p = np.array([int(p * (1 << 24)) << 8], np.uint32)
    assert R.dropout_of_words(at_p, p)[0] == np.float32(1) / (np.float32(1) - np.float32(p))
    assert R.dropout_of_words(at_p | np.uint32(0xFF), p)[0] != 0          # the low 8 bits are not used
    assert np.all(R.dropout_of_words(words[::4097], 0.0) == 1.0)          # p = 0 keeps everything, unscaled


# ------------------------------------------------------------------------------------------------ head formulas
def _head_inputs(n, d, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((n, d)) * scale).astype(np.float32) for _ in range(4)]


@pytest.mark.parametrize("gkl", [None, 0.37])
def test_head_reference_agrees_with_torch_autograd(gkl):
    n, d = 37, 5
    mu, ls, eps, dz = _head_inputs(n, d, 1)
    z, kl, zb, klb = R.head_fwd(mu, ls, eps)
    tm, tl = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (mu, ls))
    te, tg = (torch.tensor(a, dtype=torch.float64) for a in (eps, dz))
    tz = tm + te * torch.exp(tl)
    tkl = -0.5 / n ** 2 * (1 + 2 * tl - tm ** 2 - torch.exp(2 * tl)).sum()
    ((tz * tg).sum() + (1.0 if gkl is None else gkl) * tkl).backward()
    tkl = tkl.detach()
    assert np.allclose(z, tz.detach().numpy(), rtol=1e-14, atol=0) and abs(kl - float(tkl.detach())) <= 1e-14 * abs(kl)
    dmu, dls, (bm, bl) = R.head_bwd(dz, mu, ls, eps, gkl, n)
    assert np.allclose(dmu, tm.grad.numpy(), rtol=1e-13, atol=1e-16)
    assert np.allclose(dls, tl.grad.numpy(), rtol=1e-13, atol=1e-16)
    # the bounds are rounding-sized: far below the values, never zero
    for v, b in ((z, zb), (dmu, bm), (dls, bl)):
        assert (b > 0).all() and np.median(b / np.maximum(np.abs(v), 1e-30)) < 1e-5
    assert 0 < klb < 1e-5 * abs(kl)
    dmu0, dls0, _ = R.head_bwd(None, mu, ls, eps, gkl, n)                  # dz = NULL: the KL gradient alone
    g = (1.0 if gkl is None else gkl) / n ** 2
    assert np.allclose(dmu0, g * mu.astype(np.float64)) and np.allclose(dls0, g * np.expm1(2.0 * ls.astype(np.float64)))


def test_a_correctly_rounded_fp32_evaluation_stays_inside_the_bounds():
    """the kernels' sequence in numpy fp32 with a correctly rounded exp: every bound must hold with room to spare, in the
    three value regimes of tests/test_gpu_vgae_head.py"""
    f = np.float32
    for regime, (n, d) in (("a", (257, 16)), ("b", (130, 16)), ("c", (65, 17))):
        mu, ls, eps, dz = _head_inputs(n, d, 5)
        rng = np.random.default_rng(6)
        if regime == "a":
            mu, ls = mu * f(0.01), ls * f(0.01)
        if regime == "c":
            ls = rng.uniform(-8, 8, (n, d)).astype(f); mu = rng.uniform(-30, 30, (n, d)).astype(f)
        s = np.exp(ls.astype(np.float64)).astype(f)
        z32 = (eps.astype(np.float64) * s + mu).astype(f)                  # one rounding, as fmaf
        br = ((f(1) + f(2) * ls) - mu * mu) - s * s
        kl32 = f(br.astype(np.float64).sum() * (-0.5 / n ** 2))
        z, kl, zb, klb = R.head_fwd(mu, ls, eps)
        rz, rk = R.worst(z32, z, zb)[0], abs(float(kl32) - kl) / klb
        gk = f(0.37) * f(1.0 / n ** 2)
        dmu32 = (gk.astype(np.float64) * mu + dz).astype(f)
        dls32 = ((dz * eps).astype(np.float64) * s + (gk * (s * s - f(1)))).astype(f)
        dmu, dls, (bm, bl) = R.head_bwd(dz, mu, ls, eps, np.float32(0.37), n)
        rm, rl = R.worst(dmu32, dmu, bm)[0], R.worst(dls32, dls, bl)[0]
        print(f"regime {regime}: z {rz:.3f} kl {rk:.3f} (relative KL error {abs(float(kl32) - kl) / abs(kl):.2e}) "
              f"dmu {rm:.3f} dls {rl:.3f}")
        assert max(rz, rk, rm, rl) <= 1.0


def test_split_and_column_sums():
    rng = np.random.default_rng(2)
    z = (rng.standard_normal((130, 16)) * 3).astype(np.float32)
    hi, lo = R.bf16_split(z)
    back = (hi.astype(np.uint32) << 16).view(np.float32).astype(np.float64) + \
        (lo.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    assert np.abs(back - z).max() <= 2.0 ** -16 * np.abs(z).max()
    assert np.array_equal(hi, (torch.from_numpy(z).bfloat16().view(torch.int16).numpy().view(np.uint16)))
    sums, bound = R.block_colsums(z)
    assert sums.shape == (3, 16) and np.allclose(sums[2], z[128:].astype(np.float64).sum(0)) and (bound < 1e-11).all()
    P = R.head_prep(z, z * 0.1, z)
    assert P["blocks"] == 3 and abs(P["kl_partial"].sum() * (-0.5 / 130 ** 2) - P["kl"]) <= 1e-15 * abs(P["kl"])


def test_worst():
    r, i = R.worst(np.array([1.0, 2.0, 3.5]), np.array([1.0, 2.0, 3.0]), np.array([0.0, 1.0, 1.0]))
    assert (r, i) == (0.5, 2)
    assert R.worst(np.array([1.0, 2.5]), np.array([1.0, 2.0]), np.array([1.0, 0.0])) == (np.inf, 1)
    assert R.worst(np.array([np.nan, 2.0]), np.array([1.0, 2.0]), 1.0)[0] == np.inf
    assert R.worst(np.zeros(0), np.zeros(0), np.zeros(0)) == (0.0, -1)


# ------------------------------------------------------------------------------------------------ argument checks
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def fwd(lib, *, mu=FAKE, ls=FAKE, ldm=16, eps=FAKE, n=8, d=16, z=FAKE, kl=FAKE, ws=FAKE, ws_bytes=8192):
    rc = lib.gae_vgae_head_fwd(mu, ls, ldm, eps, n, d, z, kl, ws, ws_bytes, None)
    return rc, lib.gae_last_error().decode()


def bwd(lib, *, dz=FAKE, mu=FAKE, ls=FAKE, ldm=16, eps=FAKE, gkl=FAKE, n=8, d=16, dmu=FAKE, dls=FAKE):
    rc = lib.gae_vgae_head_bwd(dz, mu, ls, ldm, eps, gkl, n, d, dmu, dls, None)
    return rc, lib.gae_last_error().decode()


def prep(lib, *, mu=FAKE, ls=FAKE, ldm=16, eps=FAKE, n=130, d=16, z=FAKE, layout=True, max_blocks=3, DP=16, klp=FAKE,
         kl_capacity=3, blocks_out=True, zt=FAKE):
    from gae_dgl_amd import _lib
    lay = _lib.BcePrep(Zt=zt, Zhi=FAKE, Zlo=FAKE, colsum_partial=FAKE, scal=FAKE, all_pairs=0.0, max_blocks=max_blocks,
                       DP=DP, reserved=0)
    out = ctypes.c_int64(-1)
    rc = lib.gae_x_vgae_head_prep(mu, ls, ldm, eps, 0, 1, 0, None, n, d, z, ctypes.byref(lay) if layout else None, klp,
                                  kl_capacity, ctypes.byref(out) if blocks_out else None, None)
    assert out.value == -1                          # a refused call reports no block count
    return rc, lib.gae_last_error().decode()


@pytest.mark.parametrize("call,name", [(fwd, "gae_vgae_head_fwd"), (bwd, "gae_vgae_head_bwd")])
def test_head_sizes_are_refused(lib, call, name):
    for kw, word in (({"n": 0}, "n = 0"), ({"n": -3}, "n = -3"), ({"d": 0}, "d = 0"), ({"d": -1, "ldm": 0}, "d = -1"),
                     ({"ldm": 15}, "ldm = 15 < d = 16"), ({"d": 17, "ldm": 16}, "ldm = 16 < d = 17")):
        rc, msg = call(lib, **kw)
        assert rc == E_SIZE and name in msg and word in msg, (kw, rc, msg)


def test_head_null_operands_are_named(lib):
    for k, word in (("mu", "mu"), ("ls", "logstd"), ("eps", "eps"), ("z", "z"), ("kl", "kl_out"), ("ws", "workspace")):
        rc, msg = fwd(lib, **{k: None})
        assert rc == E_NULL and f"gae_vgae_head_fwd: {word} is NULL" in msg, (k, rc, msg)
    for k, word in (("mu", "mu"), ("ls", "logstd"), ("eps", "eps"), ("dmu", "dmu"), ("dls", "dlogstd")):
        rc, msg = bwd(lib, **{k: None})
        assert rc == E_NULL and f"gae_vgae_head_bwd: {word} is NULL" in msg, (k, rc, msg)


def test_head_workspace_below_8192_bytes_is_refused(lib):
    assert lib.gae_vgae_head_workspace_bytes(16 * 8) >= 8192 and lib.gae_vgae_head_workspace_bytes(-1) == E_SIZE
    for size in (8191, 0, -1):
        rc, msg = fwd(lib, ws_bytes=size)
        assert rc == E_WORKSPACE and "gae_vgae_head_fwd" in msg and f"workspace of {size} bytes" in msg and "8192" in msg


def test_prep_refusals(lib):
    for d in (15, 17, 32):
        rc, msg = prep(lib, d=d, ldm=32)
        assert rc == E_RANGE and "d = 16" in msg and f"got {d}" in msg and "gae_vgae_head_fwd" in msg, (rc, msg)
    for kw, word in (({"n": 0}, "n = 0"), ({"n": -1}, "n = -1"), ({"ldm": 12}, "ldm = 12"), ({"ldm": 18}, "ldm = 18"),
                     ({"ldm": 17}, "ldm = 17")):
        rc, msg = prep(lib, **kw)
        assert rc == E_SIZE and "gae_x_vgae_head_prep" in msg and word in msg, (kw, rc, msg)
    for kw, word in (({"mu": None}, "mu"), ({"ls": None}, "logstd"), ({"eps": None}, "eps"), ({"z": None}, "z"),
                     ({"layout": False}, "prep"), ({"klp": None}, "kl_partial"), ({"blocks_out": False}, "n_blocks_out")):
        rc, msg = prep(lib, **kw)
        assert rc == E_NULL and f"gae_x_vgae_head_prep: {word} is NULL" in msg, (kw, rc, msg)
    for k, word in (("mu", "mu"), ("ls", "logstd"), ("eps", "eps"), ("z", "z")):
        rc, msg = prep(lib, **{k: FAKE + 4})
        assert rc == E_ALIGN and f"{word} is not 16-byte aligned" in msg, (k, rc, msg)
    rc, msg = prep(lib, kl_capacity=2)                                     # n = 130: three blocks of 64 rows
    assert rc == E_WORKSPACE and "kl_capacity = 2 < 3 blocks" in msg, (rc, msg)
    rc, msg = prep(lib, max_blocks=2)
    assert rc == E_WORKSPACE and "max_blocks = 2 < 3 blocks" in msg, (rc, msg)
    rc, msg = prep(lib, n=128, max_blocks=1, kl_capacity=2)
    assert rc == E_WORKSPACE and "max_blocks = 1 < 2 blocks" in msg, (rc, msg)
    for kw in ({"DP": 32}, {"zt": None}):
        rc, msg = prep(lib, **kw)
        assert rc == E_WORKSPACE and "gae_x_decoder_bce_prep_layout" in msg, (kw, rc, msg)
