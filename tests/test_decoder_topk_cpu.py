"""K16 (gae_decoder_topk, GAE.predict_links) on the CPU: the workspace query and every argument error need no GPU,
metrics.recall_at_k is host glue, and the CLI refuses what cannot run before touching a device."""
import ctypes

import numpy as np
import pytest
import torch

GAE_E_NULL, GAE_E_SIZE, GAE_E_WORKSPACE, GAE_E_RANGE = -1, -2, -5, -6
SELF, EDGES = 1, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def _query(lib, n, k, d=16, node_ptr=None, n_graphs=0, max_nodes=0):
    nb = ctypes.c_int64(-1)
    rc = lib.gae_decoder_topk(None, d, n, d, k, node_ptr, n_graphs, max_nodes, None, None, SELF, None, None, k,
                              None, ctypes.byref(nb), None)
    return rc, nb.value


def test_entry_point_declared_and_bound(lib):
    from gae_dgl_amd import _lib
    assert "gae_decoder_topk" in _lib.SIGNATURES and hasattr(lib, "gae_decoder_topk")


def test_workspace_query_without_gpu(lib):
    sizes = {}
    for n in (1, 2708, 19717, 200_000, 1_000_000):
        rc, nb = _query(lib, n, 64)
        assert rc == 0 and nb > 0, (n, rc, nb)
        sizes[n] = nb
    # O(n k splits), never O(n^2): at most linear growth, and < 1 GB at n = 10^6, k = 64
    assert sizes[1_000_000] < 1 << 30
    for n in sizes:
        assert sizes[n] <= 16 * 8 * 64 * n + 4096
    assert _query(lib, 0, 10)[0] == 0
    # a fake node_ptr pointer is never dereferenced by the query
    rc, nb = _query(lib, 4096, 10, node_ptr=ctypes.c_void_p(16), n_graphs=128, max_nodes=40)
    assert rc == 0 and nb > 0


def _call(lib, **kw):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # host memory: an argument error returns before anything is touched
    a = dict(Z=p, ldz=16, n=100, d=16, k=10, node_ptr=None, n_graphs=0, max_nodes=0, indptr=p, indices=p,
             flags=SELF | EDGES, score=p, index=p, ldo=10, ws=p, nbytes=1 << 40)
    a.update(kw)
    nb = ctypes.c_int64(a["nbytes"])
    return lib.gae_decoder_topk(a["Z"], a["ldz"], a["n"], a["d"], a["k"], a["node_ptr"], a["n_graphs"],
                                a["max_nodes"], a["indptr"], a["indices"], a["flags"], a["score"], a["index"],
                                a["ldo"], a["ws"], ctypes.byref(nb), None)


@pytest.mark.parametrize("kw,code,text", [
    (dict(k=0), GAE_E_RANGE, b"k = 0"),
    (dict(k=65, ldo=65), GAE_E_RANGE, b"k = 65"),
    (dict(d=0, ldz=1), GAE_E_RANGE, b"d = 0"),
    (dict(d=257, ldz=300), GAE_E_RANGE, b"d = 257"),
    (dict(n=-1), GAE_E_SIZE, b"negative"),
    (dict(ldz=15), GAE_E_SIZE, b"leading dimension"),
    (dict(ldo=9), GAE_E_SIZE, b"leading dimension"),
    (dict(Z=None), GAE_E_NULL, b"Z is NULL"),
    (dict(score=None), GAE_E_NULL, b"NULL"),
    (dict(index=None), GAE_E_NULL, b"NULL"),
    (dict(indptr=None), GAE_E_NULL, b"without a CSR"),
    (dict(indices=None), GAE_E_NULL, b"without a CSR"),
    (dict(n=1 << 31), GAE_E_SIZE, b"int32"),
    (dict(flags=8), GAE_E_RANGE, b"flags"),
    (dict(nbytes=8), GAE_E_WORKSPACE, b"workspace"),
])
def test_argument_errors_without_gpu(lib, kw, code, text):
    assert _call(lib, **kw) == code
    assert text in lib.gae_last_error()


def test_no_csr_needed_without_edge_exclusion(lib):
    # not an error: the flags ask for no CSR (the call would launch, so only the query form is run here)
    nb = ctypes.c_int64(0)
    assert lib.gae_decoder_topk(None, 16, 100, 16, 10, None, 0, 0, None, None, SELF, None, None, 10, None,
                                ctypes.byref(nb), None) == 0


def test_ops_refuse_cpu_tensors():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    with pytest.raises(GaeHipError):
        ops.decoder_topk(torch.randn(10, 4), 3)
    with pytest.raises(ValueError):
        ops.decoder_topk(torch.randn(10, 4), 3, scope="all")


def test_recall_at_k_hand_built():
    from gae_dgl_amd import metrics
    index = torch.tensor([[1, 2], [3, -1], [-1, -1], [0, -1]])
    # (0, 1): 1 in row 0; (2, 0): 2 in row 0 -- found through the other orientation; (2, 3): nowhere; (3, 1): 3 in row 1
    assert metrics.recall_at_k(index, np.array([[0, 2, 2, 3], [1, 0, 3, 1]])) == pytest.approx(3 / 4)
    # duplicates and both directions of one pair count once
    assert metrics.recall_at_k(index, np.array([[0, 1, 0, 2], [1, 0, 1, 3]])) == pytest.approx(1 / 2)
    # padding (-1) matches nothing, also not a node -1 pair
    assert metrics.recall_at_k(index, np.array([[2], [3]])) == 0.0
    assert np.isnan(metrics.recall_at_k(index, np.zeros((2, 0), dtype=np.int64)))
    assert metrics.recall_at_k(torch.full((3, 2), -1), np.array([[0], [1]])) == 0.0


@pytest.mark.parametrize("extra,text", [(["--topk", "10"], "--topk needs --eval"),
                                        (["--topk", "0", "--eval"], "K must lie in 1..64"),
                                        (["--topk", "65", "--eval"], "K must lie in 1..64"),
                                        (["--topk_out", "x.npz"], "--topk_out needs --topk K")])
def test_cli_refuses_topk_combinations(extra, text, capsys, monkeypatch):
    from gae_dgl_amd import train_transductive as TT
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was touched"))
    with pytest.raises(SystemExit) as e:
        TT.main(["--dataset", "cora"] + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_cli_accepts_topk():
    from gae_dgl_amd import train_transductive as TT
    a = TT.parse_args(["--topk", "10", "--eval"])
    assert a.topk == 10 and a.topk_out is None
    a = TT.parse_args(["--topk", "64", "--topk_out", "t.npz"])
    assert a.topk == 64 and a.topk_out == "t.npz"
    assert TT.parse_args([]).topk is None
