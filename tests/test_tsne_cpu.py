"""K29 without a GPU: tests/tsne_ref.py against closed forms and its own finite differences, the Philox start against
words worked out with the scalar Philox of tests/sampled_ref.py, the symmetrisation (the reference's and ops'), the
choices the GPU tests rest on (rows the trajectory filter leaves out, the end-to-end run's purity and KL),
metrics.neighbourhood_preservation, and the C ABI's argument errors, size query and symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tsne_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAE_E_NULL, GAE_E_SIZE, GAE_E_WORKSPACE, GAE_E_RANGE = -1, -2, -5, -6
NEW = ["gae_tsne_chunk", "gae_tsne_workspace_bytes", "gae_tsne_init", "gae_tsne_affinities", "gae_tsne_repulsion",
       "gae_tsne_update"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the reference against closed forms
def test_two_points():
    """P = [[0, 1/2], [1/2, 0]], y = (0, 0), (a, 0): q = 1 / (1 + a^2), Z = 2 q, Q = P, so KL = 0 and
    g_0 = 4 (alpha q a / 2 - q a / 2) (-1) = -2 q a (alpha - 1) along x, g_1 = -g_0"""
    P = np.array([[0.0, 0.5], [0.5, 0.0]])
    for a in (0.3, 2.0):
        Y = np.array([[0.0, 0.0], [a, 0.0]])
        q = 1.0 / (1.0 + a * a)
        assert R.kl(Y, P) == pytest.approx(0.0, abs=1e-15)
        for alpha in (1.0, 12.0):
            r = R.gradient(Y, P, alpha)
            assert r["Z"] == pytest.approx(2 * q, rel=1e-15)
            want = np.array([[-2 * q * a * (alpha - 1), 0.0], [2 * q * a * (alpha - 1), 0.0]])
            assert np.allclose(r["g"], want, rtol=1e-14, atol=1e-15)           # the two terms are ~ 0.3: a few ulp of them
            assert np.allclose(r["A"], q * q * a, rtol=1e-14)
    part, A = R.repulsion_partials(Y, chunk=1)                 # one column per chunk: chunk 0 of row 0 is the diagonal
    assert part.shape == (2, 3, 2) and part[0, :, 0].tolist() == [0.0, 0.0, 0.0] and part[1, 2, 0] == q


def test_equilateral_triangle_has_no_gradient():
    Y = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, np.sqrt(0.75)]]) * 1.7
    P = (np.ones((3, 3)) - np.eye(3)) / 6.0
    r = R.gradient(Y, P, 1.0)
    assert np.abs(r["g"]).max() < 1e-15 and R.kl(Y, P) == pytest.approx(0.0, abs=1e-15)
    assert np.abs(R.gradient(Y, P, 12.0)["g"]).max() > 0.1     # exaggerated, the points pull together


def small_case(n=12, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 4)).astype(np.float32)
    idx, d2 = R.knn_brute(X, 5)
    p, perp = R.affinities(idx, d2, 3.0)
    return idx, p, perp, R.symmetrise(idx, p), rng.standard_normal((n, 2))


def test_gradient_is_the_derivative_of_the_kl():
    """central finite differences of the reference KL at n = 12: h = 1e-6, error O(h^2) + 1e-16 / h"""
    _, _, _, P, Y = small_case()
    g = R.gradient(Y, P, 1.0)["g"]
    h = 1e-6
    for i in range(12):
        for c in range(2):
            Yp, Ym = Y.copy(), Y.copy()
            Yp[i, c] += h
            Ym[i, c] -= h
            assert (R.kl(Yp, P) - R.kl(Ym, P)) / (2 * h) == pytest.approx(g[i, c], abs=2e-9)


def test_affinities_reach_the_perplexity_and_limits():
    idx, p, perp, _, _ = small_case()
    assert np.allclose(perp, 3.0, rtol=1e-12) and np.allclose(p.sum(1), 1.0, rtol=1e-14)
    index = np.array([[1, 2, 3, 4], [0, 2, 3, -1], [5, -1, -1, -1], [-1, -1, -1, -1], [0, 1, 2, 3]], np.int32)
    d2 = np.array([[1, 1, 1, 1], [1, 2, 3, np.inf], [7, np.inf, np.inf, np.inf], [np.inf] * 4, [2, 2, 5, 9]], np.float32)
    p, perp = R.affinities(index, d2, 1.5)
    assert np.allclose(p[0], 0.25) and perp[0] == pytest.approx(4.0)           # all equal: uniform, the target is out of reach
    assert p[1, 3] == 0.0 and perp[1] == pytest.approx(1.5, rel=1e-12)
    assert p[2].tolist() == [1.0, 0.0, 0.0, 0.0] and perp[2] == 1.0            # fewer than 2 neighbours
    assert p[3].tolist() == [0.0] * 4 and perp[3] == 0.0
    assert np.allclose(p[4], [0.5, 0.5, 0.0, 0.0]) and perp[4] == pytest.approx(2.0)     # a tie at the minimum: its limit


def test_step_rule():
    P = np.array([[0.0, 0.5], [0.5, 0.0]])
    Y = np.array([[0.0, 0.0], [1.0, 0.0]])
    v = np.array([[0.1, 0.0], [0.1, 0.0]])
    gains = np.full((2, 2), 0.0125)
    Y1, v1, g1, g = R.step(Y, v, gains, P, 12.0, 0.5, 10.0)
    assert g[0, 0] < 0 < g[1, 0] and g[0, 1] == 0 == g[1, 1]
    # row 0: sign(g) != sign(v) -> + 0.2; row 1: equal -> x 0.8 and the floor; y: both signs 0 -> x 0.8 and the floor
    assert np.allclose(g1, [[0.2125, 0.01], [0.01, 0.01]])
    assert np.allclose(v1, 0.5 * v - 10.0 * g1 * g) and np.allclose(Y1, Y + v1)


# ------------------------------------------------------------------ the start
def test_init_against_worked_philox_words():
    """word 0 of philox4x32_10(ctr = 2 i + c, draw = 0, seed ^ GAE_TSNE_KEY_XOR), worked out with the scalar
    restatement of tests/sampled_ref.py"""
    from sampled_ref import philox4x32_10
    words = {0: {0: 0x27039ef3, 1: 0x3e5cd911, 2: 0xd455c86e, 7: 0x8acc3d35},
             5: {0: 0x8506f7a8, 1: 0x263ca93e, 2: 0xcd6097e0, 7: 0x353d565c}}
    for seed, table in words.items():
        Y = R.init(4, seed)
        assert Y.dtype == np.float32 and Y.shape == (4, 2)
        for e, w in table.items():
            assert philox4x32_10(e, 0, seed ^ R.KEY_XOR)[0] == w
            m = w >> 8
            want = np.float32((2 * m - (1 << 24)) / float(1 << 24)) * np.float32(1e-4)       # (2 u - 1) exact, one rounding
            assert Y[e // 2, e % 2] == want
    assert np.abs(R.init(1000, 9)).max() <= 1e-4 and abs(float(R.init(1000, 9).mean())) < 1e-5


# ------------------------------------------------------------------ the symmetrisation
def test_symmetrisation_sums_to_one_and_is_symmetric():
    idx, p, _, P, _ = small_case()
    assert np.array_equal(P, P.T) and P.sum() == pytest.approx(1.0, rel=1e-14) and (np.diag(P) == 0).all()
    from gae_dgl_amd import ops
    p32 = p.astype(np.float32)
    indptr, indices, values = ops.tsne_symmetrise(torch.from_numpy(idx), torch.from_numpy(p32))       # torch plumbing: runs anywhere
    want = R.symmetrise(idx, p32)
    ip, ix, vv = R.csr_of(want.astype(np.float32).astype(np.float64))
    assert indptr.dtype == torch.int32 and np.array_equal(indptr.numpy(), ip) and np.array_equal(indices.numpy(), ix)
    assert np.array_equal(values.numpy(), vv)                  # merged in fp64, rounded once
    dense = np.zeros_like(want)
    dense[np.repeat(np.arange(12), np.diff(ip)), ix] = values.numpy()
    assert np.array_equal(dense, dense.T) and dense.sum() == pytest.approx(1.0, rel=1e-6)


def test_symmetrisation_drops_padding():
    from gae_dgl_amd import ops
    index = torch.tensor([[1, 2], [0, -1], [0, 1]], dtype=torch.int32)
    p = torch.tensor([[0.75, 0.25], [1.0, 0.0], [0.5, 0.5]])
    indptr, indices, values = ops.tsne_symmetrise(index, p)
    assert indptr.tolist() == [0, 2, 4, 6] and indices.tolist() == [1, 2, 0, 2, 0, 1]
    assert np.allclose(values.numpy(), np.array([1.75, 0.75, 1.75, 0.5, 0.75, 0.5]) / 6.0)


# ------------------------------------------------------------------ what the GPU tests rest on
@pytest.mark.parametrize("n", [300, 2708])
def test_trajectory_filter_leaves_out_at_most_two_percent(n):
    """the rows a reference gradient coordinate of which comes within 1e-3 max |g| of 0 in one of the five iterations"""
    ys, keep = R.trajectory(n)
    left = int((~keep).sum())
    print(f"n = {n}: {left} rows left out ({left / n:.4f})")
    assert left <= 0.02 * n and len(ys) == 5


def test_end_to_end_reference_run():
    """seed 0 of the five pinned runs: the final KL as pinned, 10-NN label purity 1.0, KL falling once the
    exaggeration is over"""
    X, classes, P = R.end_to_end_inputs()
    e = R.END_TO_END
    Y, _, ys = R.run(R.init(e["n"], 0), P, e["n_iter"], R.auto_eta(e["n"]), keep=True)
    assert R.kl(Y, P) == pytest.approx(R.END_TO_END_KL[0], rel=1e-9)
    assert R.label_purity(Y, classes) == 1.0
    curve = [R.kl(ys[i], P) for i in (259, 269, 279, 289, 299)]
    assert all(a > b for a, b in zip(curve, curve[1:]))


# ------------------------------------------------------------------ metrics
def test_neighbourhood_preservation_on_hand_made_tables():
    from gae_dgl_amd import metrics
    a = torch.tensor([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]], dtype=torch.int32)
    assert metrics.neighbourhood_preservation(a, a) == 1.0
    assert metrics.neighbourhood_preservation(a, a.flip(1)) == 1.0             # sets, not ranks
    b = torch.tensor([[1, 2, 4], [4, 5, 6], [3, 0, 5], [7, 8, -1]], dtype=torch.int32)
    assert metrics.neighbourhood_preservation(a, b) == pytest.approx((2 / 3 + 0 + 2 / 3 + 0) / 4)
    c = torch.tensor([[1, -1, -1], [-1, -1, -1], [3, 0, -1], [2, -1, -1]], dtype=torch.int32)      # padding never matches
    assert metrics.neighbourhood_preservation(c, b) == pytest.approx((1 + 1 + 0) / 3)               # row 1 has no neighbours
    assert metrics.neighbourhood_preservation(c, b, chunk_rows=1) == pytest.approx(2 / 3)
    assert np.isnan(metrics.neighbourhood_preservation(c[1:2], b[1:2]))
    with pytest.raises(ValueError):
        metrics.neighbourhood_preservation(a, b[:3])


# ------------------------------------------------------------------ the C ABI
def test_new_symbols_in_header_library_and_signatures(lib):
    from gae_dgl_amd import _lib
    seams = open(os.path.join(ROOT, "include", "gae_hip_experimental.h")).read()
    core = open(os.path.join(ROOT, "include", "gae_hip.h")).read()
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, seams) and not re.search(r"\b%s\s*\(" % s, core), s
        assert s in _lib.SIGNATURES and hasattr(lib, s), s
    assert "gae_tsne_status" in seams and _lib.TSNE_STATUS_WORDS * 8 == 64


def up256(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("n,nnz,want", [(300, 0, 16128), (2708, 100000, 423936), (249455, 12345678, 98808832)])
def test_workspace_bytes_are_pinned(lib, n, nnz, want):
    chunk = R.chunk_of(n)
    chunks = -(-n // chunk)
    assert lib.gae_tsne_chunk(n) == chunk
    reduce_blocks = -(-n // (256 if chunks <= 32 else 4))
    update_blocks = -(-n // 256)
    layout = (up256(12 * n * chunks) + 2 * up256(8 * n) + up256(8 * n) + up256(4 * reduce_blocks) + 2 * up256(8 * update_blocks)
              + up256(4 * update_blocks))
    assert lib.gae_tsne_workspace_bytes(n, nnz) == want == layout


def test_chunk_rule_and_cap(lib):
    assert [lib.gae_tsne_chunk(n) for n in (0, 1, 8192, 8193, 32768, 32769, 10 ** 6)] == [256, 256, 256, 1024, 1024, 8192, 8192]
    assert lib.gae_tsne_chunk(-1) == GAE_E_SIZE
    assert lib.gae_tsne_workspace_bytes(0, 0) > 0
    assert lib.gae_tsne_workspace_bytes(-1, 0) == GAE_E_SIZE and lib.gae_tsne_workspace_bytes(5, -1) == GAE_E_SIZE
    assert lib.gae_tsne_workspace_bytes(2 ** 31, 0) == GAE_E_SIZE and lib.gae_tsne_workspace_bytes(5, 2 ** 31) == GAE_E_SIZE
    assert lib.gae_tsne_workspace_bytes(3_000_000, 0) == GAE_E_SIZE and b"above the cap" in lib.gae_last_error()
    assert lib.gae_tsne_workspace_bytes(2_000_000, 0) > 0       # 12 n ceil(n / 8192) = 5.9e9 bytes: below 2^33


def test_argument_errors_need_no_gpu(lib):
    """every error below returns before anything is dereferenced or launched: the pointers are host dummies"""
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = 1 << 40
    # init
    assert lib.gae_tsne_init(None, 2, 5, 0, None) == GAE_E_NULL
    assert lib.gae_tsne_init(p, 1, 5, 0, None) == GAE_E_SIZE
    assert lib.gae_tsne_init(p, 2, -1, 0, None) == GAE_E_SIZE
    # affinities
    aff = lambda *a: lib.gae_tsne_affinities(*a, None)
    assert aff(p, p, 8, -1, 8, 3.0, p, 8, p) == GAE_E_SIZE
    assert aff(p, p, 65, 5, 65, 3.0, p, 65, p) == GAE_E_RANGE and b"k = 65" in lib.gae_last_error()
    assert aff(p, p, 8, 5, 0, 3.0, p, 8, p) == GAE_E_RANGE
    assert aff(p, p, 8, 5, 8, 8.0, p, 8, p) == GAE_E_RANGE and b"perplexity" in lib.gae_last_error()
    assert aff(p, p, 8, 5, 8, 0.5, p, 8, p) == GAE_E_RANGE
    assert aff(p, p, 8, 5, 8, float("nan"), p, 8, p) == GAE_E_RANGE
    assert aff(p, p, 1, 5, 1, 1.0, p, 1, p) == GAE_E_RANGE                       # k = 1 admits no perplexity
    assert aff(p, p, 7, 5, 8, 3.0, p, 8, p) == GAE_E_SIZE and aff(p, p, 8, 5, 8, 3.0, p, 7, p) == GAE_E_SIZE
    for hole in range(4):
        ptrs = [p, p, p, p]
        ptrs[hole] = None
        assert aff(ptrs[0], ptrs[1], 8, 5, 8, 3.0, ptrs[2], 8, ptrs[3]) == GAE_E_NULL
    # repulsion
    rep = lambda Y, ldy, n, lo, hi, ws, nb: lib.gae_tsne_repulsion(Y, ldy, n, lo, hi, None, ws, nb, None)
    assert rep(p, 2, -1, 0, 0, p, big) == GAE_E_SIZE
    assert rep(p, 2, 3_000_000, 0, 1, p, big) == GAE_E_SIZE
    assert rep(p, 2, 300, 0, 3, p, big) == GAE_E_RANGE and rep(p, 2, 300, 2, 1, p, big) == GAE_E_RANGE
    assert rep(p, 2, 300, -1, 1, p, big) == GAE_E_RANGE
    assert rep(None, 2, 300, 0, 2, p, big) == GAE_E_NULL and rep(p, 1, 300, 0, 2, p, big) == GAE_E_SIZE
    assert rep(p, 2, 300, 0, 2, None, big) == GAE_E_NULL
    assert rep(p, 2, 300, 0, 2, p, 16127) == GAE_E_WORKSPACE
    # update
    def upd(Y=p, ldy=2, n=300, indptr=p, indices=p, P=p, nnz=10, vel=p, gains=p, alpha=12.0, mu=0.5, eta=50.0, mgn=1e-7,
            status=p, ws=p, nb=big):
        return lib.gae_tsne_update(Y, ldy, n, indptr, indices, P, nnz, vel, gains, alpha, mu, eta, mgn, status, ws, nb, None)
    assert upd(n=-1) == GAE_E_SIZE and upd(nnz=-1) == GAE_E_SIZE and upd(n=1) == GAE_E_SIZE and upd(n=0) == GAE_E_SIZE
    assert upd(alpha=0.0) == GAE_E_RANGE and upd(mu=1.0) == GAE_E_RANGE and upd(mu=-0.1) == GAE_E_RANGE
    assert upd(eta=0.0) == GAE_E_RANGE and upd(mgn=float("nan")) == GAE_E_RANGE and upd(alpha=float("nan")) == GAE_E_RANGE
    assert upd(ldy=1) == GAE_E_SIZE
    for name in ("Y", "indptr", "indices", "P", "vel", "gains", "status", "ws"):
        assert upd(**{name: None}) == GAE_E_NULL, name
    assert upd(nb=16127) == GAE_E_WORKSPACE


def test_host_wrapper_refuses_without_a_gpu():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    with pytest.raises(GaeHipError):
        ops.tsne(torch.zeros(10, 4))                           # a CPU tensor: no fallback
    with pytest.raises(GaeHipError):
        ops.tsne_affinities(torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3), 2.0)
    for bad in (dict(perplexity=0.5), dict(n_iter=-1), dict(check_every=0), dict(learning_rate=0.0), dict(metric="dot"),
                dict(min_grad_norm=-1.0), dict(early_exaggeration=0.0)):
        with pytest.raises(ValueError):
            ops.tsne(torch.zeros(10, 4), **bad)
