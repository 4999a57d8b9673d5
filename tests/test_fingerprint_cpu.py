"""K33 / K34 without a GPU: the numpy restatement tests/fingerprint_ref.py against the definition's anchors and its
invariances, the torch helpers on host tensors, the argument errors of both entry points (returned before anything is
launched) and the refusals of the ``gae_dgl_amd.fingerprint`` parser."""
import ctypes

import numpy as np
import pytest
import torch

import fingerprint_ref as R

E_NULL, E_SIZE, E_WORKSPACE, E_RANGE = -1, -2, -5, -6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def mols():
    from gae_dgl_amd import workloads
    gp, src, dst, X = workloads.zinc_like(40, 3)
    return gp, src, dst, X


def counts_of(gp, src, dst, X, radius=2, n_bits=1024, **kw):
    ip, ix = R.csr_of(int(gp[-1]), src, dst)
    return R.fingerprint_counts(gp, ip, ix, X, radius, n_bits, **kw)


# ------------------------------------------------------------------ the definition
def test_the_anchors():
    assert int(R.mix(R.GOLD)) == 0xe220a8397b1dcdaf
    one = np.ones((2, 1), dtype=np.float32)
    ip, ix = R.csr_of(2, [0, 1], [1, 0])
    ids = R.atom_ids([0, 2], ip, ix, one, 1)
    assert [int(v) for v in ids[0]] == [0x7fefab40868a16a4] * 2 and int(ids[0, 0]) % 64 == 36
    assert [int(v) for v in ids[1]] == [0x6e37545eeea4ba15] * 2 and int(ids[1, 0]) % 64 == 21
    ip, ix = R.csr_of(1, [], [])
    lone = R.atom_ids([0, 1], ip, ix, one[:1], 1)
    assert int(lone[1, 0]) == 0xf111c56570f8befb and int(lone[1, 0]) % 64 == 59
    c = R.fingerprint_counts([0, 2], *R.csr_of(2, [0, 1], [1, 0]), one, 1, 64)
    assert c[0, 36] == 2 and c[0, 21] == 2 and c.sum() == 4


def test_atom_permutation_and_edge_order_invariance(mols):
    gp, src, dst, X = mols
    want = counts_of(gp, src, dst, X, 3)
    rng = np.random.default_rng(0)
    perm = np.concatenate([gp[g] + rng.permutation(gp[g + 1] - gp[g]) for g in range(len(gp) - 1)])   # old -> new
    Xp = np.empty_like(X)
    Xp[perm] = X
    assert np.array_equal(counts_of(gp, perm[src], perm[dst], Xp, 3), want)
    order = rng.permutation(len(src))
    assert np.array_equal(counts_of(gp, src[order], dst[order], X, 3), want)
    assert not np.array_equal(counts_of(gp, src, dst, X[::-1].copy(), 3), want)          # (it does see the atoms)


def test_uint8_and_fp32_storage_agree_and_negative_zero_is_zero(mols):
    gp, src, dst, X = mols
    assert np.array_equal(counts_of(gp, src, dst, X.astype(np.uint8)), counts_of(gp, src, dst, X))
    Z = X.copy()
    Z[Z == 0] = -0.0
    assert np.signbit(Z).any() and np.array_equal(counts_of(gp, src, dst, Z), counts_of(gp, src, dst, X))


def test_fold_is_the_fingerprint_at_the_smaller_width(mols):
    from gae_dgl_amd import ops
    gp, src, dst, X = mols
    ip, ix = R.csr_of(int(gp[-1]), src, dst)
    c1024, c128 = (R.fingerprint_counts(gp, ip, ix, X, 2, n) for n in (1024, 128))
    b1024, b128 = (R.fingerprint_bits(gp, ip, ix, X, 2, n) for n in (1024, 128))
    assert torch.equal(ops.fingerprint_fold(torch.from_numpy(c1024), 128), torch.from_numpy(c128))
    assert torch.equal(ops.fingerprint_fold(torch.from_numpy(b1024), 128), torch.from_numpy(b128))
    assert torch.equal(ops.fingerprint_fold(torch.from_numpy(c128), 64), torch.from_numpy(c128[:, :64] + c128[:, 64:]))
    assert torch.equal(ops.fingerprint_fold(torch.from_numpy(c1024), 1024), torch.from_numpy(c1024))
    b2048 = torch.from_numpy(R.fingerprint_bits(gp, ip, ix, X, 2, 2048))
    c64 = torch.from_numpy(R.fingerprint_counts(gp, ip, ix, X, 2, 64))
    assert torch.equal(ops.fingerprint_fold(b2048, 128, counts=False), torch.from_numpy(b128))
    assert torch.equal(ops.fingerprint_fold(c64, 64, counts=True), c64)
    for bad in (lambda: ops.fingerprint_fold(c64, 64), lambda: ops.fingerprint_fold(torch.from_numpy(c128), 256),
                lambda: ops.fingerprint_fold(torch.from_numpy(c128), 96), lambda: ops.fingerprint_fold(c64.float(), 64)):
        with pytest.raises(ops.GaeHipError):
            bad()


def test_duplicate_edges_change_the_result_and_bits_are_positive_counts(mols):
    gp, src, dst, X = mols
    base = counts_of(gp, src, dst, X)
    twice = counts_of(gp, np.concatenate([src, src[:2]]), np.concatenate([dst, dst[:2]]), X)
    assert not np.array_equal(twice[0], base[0]) and np.array_equal(twice[5:], base[5:])
    ip, ix = R.csr_of(int(gp[-1]), src, dst)
    bits = R.fingerprint_bits(gp, ip, ix, X)
    from gae_dgl_amd import ops
    assert torch.equal(ops.fingerprint_unpack(torch.from_numpy(bits), torch.bool), torch.from_numpy(base > 0))
    assert base.sum(1).tolist() == (3 * np.diff(gp)).tolist()          # every (atom, r) emits once


def test_graph_ids_select_rows_and_a_bad_id_is_a_zero_row(mols):
    gp, src, dst, X = mols
    base = counts_of(gp, src, dst, X, 1, 64)
    got = counts_of(gp, src, dst, X, 1, 64, graph_ids=[7, 0, 7, -1, 40])
    assert np.array_equal(got[:3], base[[7, 0, 7]]) and not got[3:].any()


def test_unpack_on_host_tensors():
    from gae_dgl_amd import ops
    w = torch.tensor([[1, -2 ** 31], [6, 0]], dtype=torch.int32)
    u = ops.fingerprint_unpack(w)
    assert u.dtype == torch.float32 and u.shape == (2, 64)
    assert u[0].nonzero().reshape(-1).tolist() == [0, 63] and u[1].nonzero().reshape(-1).tolist() == [1, 2]
    assert ops.fingerprint_unpack(w, torch.float16).dtype == torch.float16
    assert np.array_equal(R.pack_bits(u.numpy() > 0), w.numpy())
    with pytest.raises(ops.GaeHipError):
        ops.fingerprint_unpack(w.long())


# ------------------------------------------------------------------ Tanimoto: the restatement and the fact it rests on
def test_fp32_quotients_of_fractions_up_to_4096_are_distinct_and_monotone():
    """for every c / u with u <= 4096: two different fractions never share an fp32 quotient and the quotients keep the
    exact order -- so a kernel that selects on the fp32 value selects on the fraction"""
    u = np.repeat(np.arange(1, 4097, dtype=np.int64), np.arange(2, 4098))
    c = np.arange(len(u), dtype=np.int64) - np.repeat(np.cumsum(np.arange(2, 4098)) - np.arange(2, 4098), np.arange(2, 4098))
    assert c.min() == 0 and (c <= u).all() and (c[u == 4096] == np.arange(4097)).all()
    exact = c / u                                                      # fp64: fractions differ by >= 2^-24, far above 2^-53
    q32 = c.astype(np.float32) / u.astype(np.float32)
    order = np.argsort(exact, kind="stable")
    e, q = exact[order], q32[order]
    assert (np.diff(q) >= 0).all()
    assert ((np.diff(q) == 0) == (np.diff(e) == 0)).all()


def test_tanimoto_reference_orders_ties_by_index():
    Q = np.array([[0b1111, 0]], dtype=np.int32)
    X = np.array([[0b0011, 0], [0b1111, 0], [0b1100, 0], [0, 0], [0b1111, 0], [0, 1]], dtype=np.int32)
    idx, val = R.tanimoto_knn(Q, X, 7)
    assert idx.tolist() == [[1, 4, 0, 2, 3, 5, -1]]
    assert val[0, :6].tolist() == [1.0, 1.0, 0.5, 0.5, 0.0, 0.0] and val[0, 6] == -np.inf
    assert R.tanimoto_knn(np.zeros((1, 2), np.int32), np.zeros((2, 2), np.int32), 1)[1][0, 0] == 0.0    # u = 0
    assert R.tanimoto_knn(X, X, 2, exclude_same=True)[0][1].tolist() == [4, 0]


# ------------------------------------------------------------------ argument errors need no GPU
def test_argument_errors_of_both_entry_points():
    from gae_dgl_amd import _lib
    lib = _lib.load()
    P = ctypes.c_void_p(256)                                           # never dereferenced: every call below is refused

    def fp(radius=2, n_bits=1024, counts=0, graph_ptr=P, indptr=P, indices=P, feat=P, out=P, ws=P, ldf=39, ldo=2048,
           dtype=_lib.U8, f_in=39, nbytes=1 << 30, n_nodes=10):
        return lib.gae_fingerprint_graphs(graph_ptr, 2, n_nodes, 20, indptr, indices, feat, dtype, ldf, f_in, None, 2, radius,
                                          n_bits, counts, out, ldo, ws, nbytes, None)
    assert fp(radius=9) == -6 and b"radius" in lib.gae_last_error()
    assert fp(radius=-1) == -6
    for n_bits in (96, 4096, 32, 0):
        assert fp(n_bits=n_bits) == -6 and b"n_bits" in lib.gae_last_error()
    assert fp(counts=2) == -6
    assert fp(f_in=0) == -6
    assert fp(dtype=_lib.BF16) == -4
    assert fp(ldf=38) == -2 and fp(ldo=31) == -2 and fp(counts=1, ldo=1023) == -2
    assert fp(n_nodes=-1) == -2 and fp(n_nodes=1 << 31) == -2
    for name in ("graph_ptr", "indptr", "indices", "feat", "out", "ws"):
        assert fp(**{name: None}) == -1, name
    assert fp(nbytes=16) == -5
    assert lib.gae_fingerprint_workspace_bytes(10) >= 160 and lib.gae_fingerprint_workspace_bytes(-1) == -2
    assert lib.gae_fingerprint_workspace_bytes(0) > 0

    def tn(W=32, k=10, m=5, n=7, Q=P, X=P, index=P, value=P, ws=P, ldq=64, ldx=64, ldo=64, flags=0, splits=0,
           nbytes=1 << 30):
        return lib.gae_tanimoto_knn(Q, ldq, m, X, ldx, n, W, k, flags, splits, index, value, ldo, ws, nbytes, None)
    assert tn(W=65) == -6 and b"n_words" in lib.gae_last_error()
    assert tn(W=0) == -6
    assert tn(k=65) == -6 and tn(k=0) == -6
    assert tn(splits=17) == -6 and tn(flags=2) == -6
    assert tn(ldo=9) == -2 and b"ldo" in lib.gae_last_error()
    assert tn(ldq=31) == -2 and tn(ldx=31) == -2
    assert tn(m=-1) == -2 and tn(n=1 << 31) == -2
    for name in ("Q", "X", "index", "value", "ws"):
        assert tn(**{name: None}) == -1, name
    assert tn(nbytes=16) == -5
    assert tn(m=0, Q=None, X=None, index=None, value=None) == 0        # nothing to do: no launch
    wb = lib.gae_tanimoto_knn_workspace_bytes
    assert wb(5, 7, 65, 10, 0) == -6 and wb(5, 7, 32, 65, 0) == -6 and wb(5, 7, 32, 10, 17) == -6
    assert 0 < wb(100, 1000, 32, 10, 0) <= wb(200, 1000, 32, 10, 0) <= wb(200, 2000, 32, 64, 0) <= wb(200, 2000, 32, 64, 16)


def call_tanimoto(lib, *, ldq=8, m=4, ldx=8, n=10, W=8, k=3, flags=0, splits=0, index=1 << 20, value=1 << 21, ldo=3,
                  ws=1 << 22, ws_bytes=1 << 30, Q=1 << 23, X=1 << 24):
    """gae_tanimoto_knn with made-up non-NULL addresses: an argument error must return before any of them is touched"""
    rc = lib.gae_tanimoto_knn(Q, ldq, m, X, ldx, n, W, k, flags, splits, index, value, ldo, ws, ws_bytes, None)
    return rc, lib.gae_last_error().decode()


@pytest.mark.parametrize("kw, code, text", [
    (dict(W=0), E_RANGE, "n_words = 0 outside 1..64"),
    (dict(W=65, ldq=80, ldx=80), E_RANGE, "n_words = 65 outside 1..64"),
    (dict(k=0), E_RANGE, "k = 0 outside 1..64"),
    (dict(k=65, ldo=65), E_RANGE, "k = 65 outside 1..64"),
    (dict(m=-1), E_SIZE, "negative m = -1"),
    (dict(n=-1), E_SIZE, "negative m = 4 or n = -1"),
    (dict(m=1 << 31), E_SIZE, "m = 2147483648 or n = 10 beyond int32 indices"),
    (dict(n=1 << 31), E_SIZE, "beyond int32 indices"),
    (dict(ldq=7), E_SIZE, "leading dimension too small (ldq 7 < n_words, ldx 8 < n_words or ldo 3 < k)"),
    (dict(ldx=7), E_SIZE, "ldx 7 < n_words"),
    (dict(ldo=2), E_SIZE, "ldo 2 < k"),
    (dict(flags=2), E_RANGE, "unknown flags 0x2"),
    (dict(splits=17), E_RANGE, "splits = 17 outside 0..16"),
    (dict(splits=-1), E_RANGE, "splits = -1 outside 0..16"),
    (dict(index=None), E_NULL, "index_out / value_out is NULL"),
    (dict(value=None), E_NULL, "index_out / value_out is NULL"),
    (dict(Q=None), E_NULL, "Q is NULL"),
    (dict(X=None), E_NULL, "X is NULL"),
    (dict(ws=None), E_NULL, "workspace is NULL"),
    (dict(ws_bytes=16), E_WORKSPACE, "workspace of 16 bytes, "),
    # two bad arguments: the one that is checked first is the one reported
    (dict(W=65, ldq=80, ldx=80, k=65, ldo=65), E_RANGE, "n_words = 65 outside 1..64"),
    (dict(splits=17, flags=2), E_RANGE, "splits = 17 outside 0..16"),
])
def test_tanimoto_argument_errors_come_before_any_access(lib, kw, code, text):
    rc, msg = call_tanimoto(lib, **kw)
    assert rc == code, (rc, msg)
    assert msg.startswith("gae_tanimoto_knn: ") and text in msg, msg


def test_tanimoto_workspace_query_is_a_monotone_host_function(lib):
    """the sweep of test_knn_cpu.py for K34: its blocks hold 256 queries, so the bound of the partial lists passes from
    16 m to 1024 . 256 + m between m = 17476 and 17477, and the auto split is 1 from m = 1023 . 256 + 1 on"""
    q = lib.gae_tanimoto_knn_workspace_bytes
    assert q(0, 0, 1, 1, 0) > 0 and q(100, 1000, 32, 10, 0) == q(100, 1000, 32, 10, 0)
    for splits in (0, 1, 3, 16):
        prev = 0
        for m in (0, 1, 31, 32, 33, 127, 128, 129, 4096, 17476, 17477, 249455, 261888, 261889, 262144, 262145, 10 ** 6,
                  2 ** 31 - 1):
            cur = q(m, 249455, 32, 10, splits)
            assert cur >= prev > -1, (m, splits)
            prev = cur
        prev = 0
        for n in (0, 1, 255, 256, 257, 4096, 249455, 2 ** 31 - 1):
            cur = q(4096, n, 32, 10, splits)
            assert cur >= prev > -1, (n, splits)
            prev = cur
        prev = 0
        for k in range(1, 65):
            cur = q(4096, 249455, 32, k, splits)
            assert cur >= prev > -1, (k, splits)
            prev = cur
    prev = 0
    for splits in range(1, 17):
        cur = q(4096, 249455, 32, 10, splits)
        assert cur > prev
        prev = cur
    # never the m x n matrix: linear in n + m k splits
    assert q(249455, 249455, 32, 10, 0) < 4 * 249455 + 8 * 10 * 16 * 249455 + 4096
    assert q(10, 10, 0, 1, 0) == E_RANGE and q(10, 10, 8, 65, 0) == E_RANGE and q(-1, 10, 8, 1, 0) == E_SIZE
    assert q(10, 10, 8, 1, 17) == E_RANGE and b"splits = 17" in lib.gae_last_error()


def test_ops_refuse_host_tensors_and_bad_options():
    from gae_dgl_amd import ops
    gp = torch.tensor([0, 2]); ip = torch.tensor([0, 1, 2], dtype=torch.int32); ix = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(ops.GaeHipError):
        ops.fingerprint_graphs(gp, ip, ix, torch.ones(2, 1))           # host tensors: no CPU fallback
    for bad in (dict(radius=9), dict(n_bits=96), dict(n_bits=4096), dict(radius=1.5)):
        with pytest.raises(ops.GaeHipError):
            ops.fingerprint_graphs(gp, ip, ix, torch.ones(2, 1), **bad)
    with pytest.raises(ops.GaeHipError):
        ops.tanimoto_knn(torch.zeros(3, 2, dtype=torch.int32), k=1)
    with pytest.raises(ValueError):
        ops.tanimoto_knn(torch.zeros(3, 2, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.tanimoto_knn(torch.zeros(3, 2, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int32), k=1, exclude_self=True)


# ------------------------------------------------------------------ the script's parser
def test_the_script_refuses_impossible_combinations(tmp_path, capsys):
    from gae_dgl_amd import fingerprint as F
    y = str(tmp_path / "y.npy")
    np.save(y, np.zeros(3))
    base = ["--synthetic", "3", "--out", str(tmp_path / "fp.npy")]
    ok = F.parse_args(base + ["--neighbours", "5", "--targets", y, "--ridge", "--forest", "--mlp", "--counts"])
    assert ok.forest == 100 and ok.mlp == [] and ok.ridge and ok.n_bits == 1024 and ok.radius == 2
    assert F.parse_args(base + ["--forest", "10", "--targets", y]).forest == 10
    refused = [
        ["--out", "x.npy"],                                            # neither a file nor --synthetic
        ["--synthetic", "3", "-d", "a.npz", "--out", "x.npy"],         # both
        ["--synthetic", "3"],                                          # no --out
        base + ["--n_bits", "96"], base + ["--n_bits", "4096"], base + ["--radius", "9"], base + ["--radius", "-1"],
        base + ["--neighbours", "0"], base + ["--neighbours", "65"],
        base + ["--neighbours_out", "nn.npz"], base + ["--labels", y], base + ["--targets", y],
        base + ["--ridge"], base + ["--forest"], base + ["--mlp"],
        base + ["--forest", "0", "--targets", y], base + ["--mlp", "1", "2", "3", "--targets", y],
        base + ["--mlp", "500", "--targets", y],
        base + ["--ridge", "--targets", str(tmp_path / "missing.npy")],
        base + ["--neighbours", "3", "--labels", str(tmp_path / "missing.npy")],
    ]
    for argv in refused:
        with pytest.raises(SystemExit):
            F.parse_args(argv)
        assert "error:" in capsys.readouterr().err, argv
