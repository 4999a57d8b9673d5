"""K18 (gae_decoder_rank, GAE.rank_links) on the CPU: the workspace query and every argument error need no GPU,
metrics.rank_metrics is host glue, tests/rank_ref.py is checked against a literal triple loop, and the CLI refuses what
cannot run before touching a device."""
import ctypes
import math

import numpy as np
import pytest
import torch

from rank_ref import rank_ref

GAE_E_NULL, GAE_E_SIZE, GAE_E_WORKSPACE, GAE_E_RANGE = -1, -2, -5, -6
SELF, EDGES = 1, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def _query(lib, n, m, d=16, node_ptr=None, n_graphs=0, max_nodes=0):
    nb = ctypes.c_int64(-1)
    rc = lib.gae_decoder_rank(None, d, n, d, None, None, m, node_ptr, n_graphs, max_nodes, None, None, SELF,
                              None, None, None, None, None, ctypes.byref(nb), None)
    return rc, nb.value


def test_entry_point_declared_and_bound(lib):
    from gae_dgl_amd import _lib
    assert "gae_decoder_rank" in _lib.SIGNATURES and hasattr(lib, "gae_decoder_rank")
    header = open(_lib.LIB_PATH.split("gae_dgl_amd")[0] + "include/gae_hip_experimental.h").read()
    assert "int gae_decoder_rank(" in header


def test_workspace_query_without_gpu(lib):
    sizes = {}
    for n, m in ((1, 1), (2708, 2708), (19717, 2048), (200_000, 512), (200_000, 200_000), (1_000_000, 1_000_000),
                 (1_000_000, 1)):
        rc, nb = _query(lib, n, m)
        assert rc == 0 and nb > 0, (n, m, rc, nb)
        sizes[(n, m)] = nb
        # O(m splits): at most linear in m (16 splits, three int32 per query and split), whatever n is
        assert nb <= 16 * 12 * m + 4096, (n, m, nb)
    assert sizes[(1_000_000, 1_000_000)] < 1 << 30
    assert _query(lib, 0, 10)[0] == 0 and _query(lib, 10, 0)[0] == 0 and _query(lib, 0, 0)[0] == 0
    # a fake node_ptr pointer is never dereferenced by the query
    rc, nb = _query(lib, 4096, 100, node_ptr=ctypes.c_void_p(16), n_graphs=128, max_nodes=40)
    assert rc == 0 and nb > 0


def _call(lib, **kw):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # host memory: an argument error returns before anything is touched
    a = dict(Z=p, ldz=16, n=100, d=16, src=p, dst=p, m=50, node_ptr=None, n_graphs=0, max_nodes=0, indptr=p, indices=p,
             flags=SELF | EDGES, score=p, greater=p, equal=p, cand=p, ws=p, nbytes=1 << 40)
    a.update(kw)
    nb = ctypes.c_int64(a["nbytes"])
    return lib.gae_decoder_rank(a["Z"], a["ldz"], a["n"], a["d"], a["src"], a["dst"], a["m"], a["node_ptr"],
                                a["n_graphs"], a["max_nodes"], a["indptr"], a["indices"], a["flags"], a["score"],
                                a["greater"], a["equal"], a["cand"], a["ws"], ctypes.byref(nb), None)


@pytest.mark.parametrize("kw,code,text", [
    (dict(d=0, ldz=1), GAE_E_RANGE, b"d = 0"),
    (dict(d=257, ldz=300), GAE_E_RANGE, b"d = 257"),
    (dict(n=-1), GAE_E_SIZE, b"negative"),
    (dict(m=-1), GAE_E_SIZE, b"negative"),
    (dict(ldz=15), GAE_E_SIZE, b"leading dimension"),
    (dict(Z=None), GAE_E_NULL, b"Z is NULL"),
    (dict(src=None), GAE_E_NULL, b"src / dst is NULL"),
    (dict(dst=None), GAE_E_NULL, b"src / dst is NULL"),
    (dict(score=None), GAE_E_NULL, b"NULL"),
    (dict(greater=None), GAE_E_NULL, b"NULL"),
    (dict(equal=None), GAE_E_NULL, b"NULL"),
    (dict(cand=None), GAE_E_NULL, b"NULL"),
    (dict(indptr=None), GAE_E_NULL, b"without a CSR"),
    (dict(indices=None), GAE_E_NULL, b"without a CSR"),
    (dict(n=1 << 31), GAE_E_SIZE, b"int32"),
    (dict(m=1 << 31), GAE_E_SIZE, b"queries"),
    (dict(flags=8), GAE_E_RANGE, b"flags"),
    (dict(flags=4 | SELF), GAE_E_RANGE, b"flags"),
    (dict(nbytes=8), GAE_E_WORKSPACE, b"workspace"),
])
def test_argument_errors_without_gpu(lib, kw, code, text):
    assert _call(lib, **kw) == code
    assert text in lib.gae_last_error()
    assert b"gae_decoder_rank" in lib.gae_last_error()


def test_rank_splits_knob(lib):
    """the one tuning knob: default 0 (auto), 0 .. 16, named in the header that declares the entry point"""
    v = ctypes.c_int64(-1)
    assert lib.gae_tuning_get(b"rank_splits", ctypes.byref(v)) == 0 and v.value == 0
    try:
        for s in (1, 16):
            assert lib.gae_tuning_set(b"rank_splits", s) == 0
            # the size query follows the knob: S parts of three int32 per query
            assert _query(lib, 5000, 1000)[1] == (256 if s == 1 else 256 + s * 12 * 1000)
        assert lib.gae_tuning_set(b"rank_splits", 17) == GAE_E_RANGE
        assert lib.gae_tuning_set(b"rank_splits", -1) == GAE_E_RANGE
    finally:
        assert lib.gae_tuning_set(b"rank_splits", 0) == 0


def test_ops_refuse_cpu_tensors_and_bad_pairs():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    with pytest.raises(GaeHipError):
        ops.decoder_rank(torch.randn(10, 4), np.array([[0], [1]]))
    with pytest.raises(ValueError):
        ops.decoder_rank(torch.randn(10, 4), np.array([[0], [1]]), scope="all")
    assert ops.RankResult._fields == ("score", "greater", "equal", "candidates")


# ------------------------------------------------------------------ metrics.rank_metrics
def test_rank_metrics_hand_worked():
    from gae_dgl_amd import metrics
    # ranks: 1 + 0 + 0 = 1;  1 + 2 + 2/2 = 4;  1 + 9 + 0 = 10;  1 + 0 + 3/2 = 2.5;  a query without candidates: rank 1
    greater = torch.tensor([0, 2, 9, 0, 0])
    equal = torch.tensor([0, 2, 0, 3, 0])
    cand = torch.tensor([10, 10, 9, 4, 0])
    r = metrics.rank_metrics(greater, equal, cand, ks=(1, 3, 10))
    ranks = [1, 4, 10, 2.5, 1]
    assert r["queries"] == 5
    assert r["mrr"] == pytest.approx(sum(1 / x for x in ranks) / 5)
    assert r["mean_rank"] == pytest.approx(sum(ranks) / 5)
    assert r["hits@1"] == pytest.approx(2 / 5)
    assert r["hits@3"] == pytest.approx(3 / 5)
    assert r["hits@10"] == pytest.approx(1.0)
    # auc over the four queries that have candidates: 1 - (greater + equal / 2) / candidates
    assert r["auc"] == pytest.approx((1 + (1 - 3 / 10) + (1 - 9 / 9) + (1 - 1.5 / 4)) / 4)
    # default ks
    assert set(metrics.rank_metrics(greater, equal, cand)) == {"queries", "mrr", "mean_rank", "auc", "hits@1",
                                                               "hits@10", "hits@50", "hits@100"}
    # numpy input works as well
    assert metrics.rank_metrics(greater.numpy(), equal.numpy(), cand.numpy())["mrr"] == pytest.approx(r["mrr"])


def test_rank_metrics_edge_cases():
    from gae_dgl_amd import metrics
    e = torch.zeros(0, dtype=torch.int64)
    r = metrics.rank_metrics(e, e, e)
    assert r["queries"] == 0 and all(math.isnan(r[k]) for k in ("mrr", "mean_rank", "auc", "hits@1", "hits@100"))
    z = torch.zeros(3, dtype=torch.int64)
    r = metrics.rank_metrics(z, z, z)              # no candidates anywhere: every rank is 1, the AUC is undefined
    assert r["mrr"] == 1.0 and r["hits@1"] == 1.0 and math.isnan(r["auc"])
    for bad in range(3):
        a = [torch.tensor([1, 2]), torch.tensor([0, 0]), torch.tensor([5, 5])]
        a[bad] = torch.tensor([1, -1])
        with pytest.raises(ValueError):
            metrics.rank_metrics(*a)
    with pytest.raises(ValueError):
        metrics.rank_metrics(torch.tensor([1, 2]), torch.tensor([0]), torch.tensor([5, 5]))


# ------------------------------------------------------------------ the test-side reference against a literal loop
def _literal(Z, src, dst, windows, indptr, indices, exclude_self):
    n, d = Z.shape
    out = []
    for q in range(len(src)):
        i, j = src[q], dst[q]
        if not (0 <= i < n and 0 <= j < n):
            out.append((float("nan"), -1, -1, -1))
            continue
        t = 0.0
        for f in range(d):
            t += float(Z[i, f]) * float(Z[j, f])
        g = e = c = 0
        for col in range(n):
            if col == j:
                continue
            if windows is not None and not (windows[i][0] <= col < windows[i][1]):
                continue
            if exclude_self and col == i:
                continue
            if indptr is not None and any(indices[x] == col for x in range(indptr[i], indptr[i + 1])):
                continue
            s = 0.0
            for f in range(d):
                s += float(Z[i, f]) * float(Z[col, f])
            c += 1
            g += s > t
            e += s == t
        out.append((t, g, e, c))
    return out


def test_rank_ref_against_a_literal_triple_loop():
    rng = np.random.default_rng(0)
    n, d = 12, 3
    Z = rng.integers(-2, 3, (n, d)).astype(np.float64)
    Z[7] = Z[2]                                               # ties
    rows = [[1, 2], [0, 0, 5], [], [4, 4, 4, 11], [3], [1, 6, 1], [5], [], [9, 10], [8], [8, 8], [3, 0]]
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])            # rows 1, 3, 5, 10 repeat an entry
    indices = np.array([c for r in rows for c in r], dtype=np.int64)
    windows = np.array([[0, 7]] * 7 + [[7, 12]] * 5)          # a two-member window
    #       target in the CSR row | self pair | across the window | plain | repeated source | out of range
    src = np.array([1, 3, 4, 8, 2, 9, 1, 1, 0, 12, 3])
    dst = np.array([5, 11, 4, 8, 9, 3, 0, 7, 3, 0, -1])
    for wins in (None, windows):
        for csr in (None, (indptr, indices)):
            for ex in (True, False):
                ref = _literal(Z, src, dst, wins, *(csr if csr else (None, None)), ex)
                score, greater, equal, cand = rank_ref(Z, src, dst, wins, csr, ex)
                for q, (t, g, e, c) in enumerate(ref):
                    assert (math.isnan(t) and math.isnan(score[q])) or t == score[q], q
                    assert (greater[q], equal[q], cand[q]) == (g, e, c), (q, wins is None, csr is None, ex)
    # the repeated entry counts once: row 3 = [4, 4, 4, 11], query (3, 11) filters {4} and exempts the target 11
    _, _, _, cand = rank_ref(Z, [3], [11], None, (indptr, indices), True)
    assert cand[0] == n - 1 - 1 - 1                           # minus self, minus node 4, minus the target


# ------------------------------------------------------------------ CLI
def test_cli_refuses_rank_without_eval(capsys, monkeypatch):
    from gae_dgl_amd import train_transductive as TT
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was touched"))
    with pytest.raises(SystemExit) as e:
        TT.main(["--dataset", "cora", "--rank"])
    assert e.value.code == 2
    assert "--rank needs --eval" in capsys.readouterr().err


def test_cli_accepts_rank():
    from gae_dgl_amd import train_transductive as TT
    assert TT.parse_args(["--eval", "--rank"]).rank is True
    assert TT.parse_args(["--eval"]).rank is False
