"""K22 (gae_decoder_threshold_count / _fill, GAE.reconstruct) on the CPU: the workspace query and every argument error
need no GPU, metrics.reconstruction_metrics is host glue, the probability-to-logit helper is arithmetic, and the CLI
refuses what cannot run before touching a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

GAE_E_NULL, GAE_E_SIZE, GAE_E_WORKSPACE, GAE_E_RANGE = -1, -2, -5, -6
SELF, EDGES = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("gae_decoder_threshold_count", "gae_decoder_threshold_fill")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def test_entry_points_declared_exported_and_bound(lib):
    from gae_dgl_amd import _lib
    seams = open(os.path.join(ROOT, "include", "gae_hip_experimental.h")).read()
    core = open(os.path.join(ROOT, "include", "gae_hip.h")).read()
    for s in SYMBOLS:
        assert re.search(rf"\bint {s}\s*\(", seams), s
        assert s not in core                               # the boundary header is full (test_abi_cpu.py)
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    assert len(_lib.SIGNATURES[SYMBOLS[0]][1]) == 16 and len(_lib.SIGNATURES[SYMBOLS[1]][1]) == 19


def _query(lib, n, d=16, splits=0, node_ptr=None, n_graphs=0, max_nodes=0, fill=False, threshold=0.0):
    nb = ctypes.c_int64(-1)
    if fill:
        rc = lib.gae_decoder_threshold_fill(None, d, n, d, threshold, node_ptr, n_graphs, max_nodes, None, None, SELF,
                                            splits, None, None, None, 0, None, ctypes.byref(nb), None)
    else:
        rc = lib.gae_decoder_threshold_count(None, d, n, d, threshold, node_ptr, n_graphs, max_nodes, None, None, SELF,
                                             splits, None, None, ctypes.byref(nb), None)
    return rc, nb.value


def test_workspace_query_without_gpu(lib):
    sizes = {}
    for n in (0, 1, 2708, 19717, 1_000_000):
        rc, nb = _query(lib, n)
        assert rc == 0 and nb > 0, (n, rc, nb)
        assert _query(lib, n, fill=True) == (0, nb)       # both calls ask for the same workspace
        sizes[n] = nb
        for s in (1, 16):
            rc, nb_s = _query(lib, n, splits=s)
            # O(n splits): 12 bytes per (row, split) + 8 per 1024 of them + the header, never O(n^2) or O(output)
            assert rc == 0 and nb_s <= 12 * n * s + 8 * (n * s // 1024 + 2) + 512, (n, s, nb_s)
    for n in sizes:                                        # at most linear in n, whatever the auto split picks
        assert sizes[n] <= 16 * 12 * n + 16 * n // 64 + 1024
    assert sizes[1_000_000] < 1 << 28
    # the threshold does not size anything: the workspace is not O(output)
    assert _query(lib, 19717, threshold=float("-inf"))[1] == sizes[19717] == _query(lib, 19717, threshold=50.0)[1]
    # a fake node_ptr pointer is never dereferenced by the query
    rc, nb = _query(lib, 4096, node_ptr=ctypes.c_void_p(16), n_graphs=128, max_nodes=40)
    assert rc == 0 and nb > 0
    assert _query(lib, 4096, node_ptr=ctypes.c_void_p(16), n_graphs=128, max_nodes=40, fill=True) == (0, nb)


def _call(lib, which, **kw):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)       # host memory: an argument error returns before anything is touched
    a = dict(Z=p, ldz=16, n=100, d=16, threshold=0.0, node_ptr=None, n_graphs=0, max_nodes=0, indptr=p, indices=p,
             flags=SELF | EDGES, splits=0, row_ptr=p, index=p, score=p, capacity=10, ws=p, nbytes=1 << 40)
    a.update(kw)
    nb = ctypes.c_int64(a["nbytes"])
    head = (a["Z"], a["ldz"], a["n"], a["d"], a["threshold"], a["node_ptr"], a["n_graphs"], a["max_nodes"], a["indptr"],
            a["indices"], a["flags"], a["splits"])
    if which == "count":
        return lib.gae_decoder_threshold_count(*head, a["row_ptr"], a["ws"], ctypes.byref(nb), None)
    return lib.gae_decoder_threshold_fill(*head, a["row_ptr"], a["index"], a["score"], a["capacity"], a["ws"],
                                          ctypes.byref(nb), None)


COMMON_ERRORS = [
    (dict(threshold=float("nan")), GAE_E_RANGE, b"NaN"),
    (dict(d=0, ldz=1), GAE_E_RANGE, b"d = 0"),
    (dict(d=257, ldz=300), GAE_E_RANGE, b"d = 257"),
    (dict(n=-1), GAE_E_SIZE, b"negative"),
    (dict(n=1 << 31), GAE_E_SIZE, b"int32"),
    (dict(ldz=15), GAE_E_SIZE, b"leading dimension"),
    (dict(flags=8), GAE_E_RANGE, b"flags"),
    (dict(indptr=None), GAE_E_NULL, b"without a CSR"),
    (dict(indices=None), GAE_E_NULL, b"without a CSR"),
    (dict(splits=-1), GAE_E_RANGE, b"splits = -1"),
    (dict(splits=17), GAE_E_RANGE, b"splits = 17"),
    (dict(Z=None), GAE_E_NULL, b"Z is NULL"),
    (dict(row_ptr=None), GAE_E_NULL, b"NULL"),
    (dict(nbytes=8), GAE_E_WORKSPACE, b"workspace"),
]


@pytest.mark.parametrize("which", ["count", "fill"])
@pytest.mark.parametrize("kw,code,text", COMMON_ERRORS)
def test_argument_errors_without_gpu(lib, which, kw, code, text):
    assert _call(lib, which, **kw) == code
    assert text in lib.gae_last_error() and f"gae_decoder_threshold_{which}".encode() in lib.gae_last_error()


@pytest.mark.parametrize("kw,code,text", [
    (dict(index=None), GAE_E_NULL, b"index_out / score_out is NULL"),
    (dict(score=None), GAE_E_NULL, b"index_out / score_out is NULL"),
    (dict(capacity=-1), GAE_E_SIZE, b"negative capacity"),
])
def test_fill_argument_errors_without_gpu(lib, kw, code, text):
    assert _call(lib, "fill", **kw) == code
    assert text in lib.gae_last_error()


def test_calls_that_launch_nothing_succeed_without_gpu(lib):
    # the fill of an empty list: capacity 0 needs no output arrays and launches nothing
    assert _call(lib, "fill", capacity=0, index=None, score=None) == 0
    assert _call(lib, "fill", n=0, Z=None) == 0
    # not an error: the flags ask for no CSR (the call would launch, so only the query form is run here)
    assert _query(lib, 100)[0] == 0


def test_ops_refuse_cpu_tensors_and_bad_scope():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    with pytest.raises(GaeHipError):
        ops.decoder_threshold(torch.randn(10, 4), 0.0)
    with pytest.raises(ValueError):
        ops.decoder_threshold(torch.randn(10, 4), 0.0, scope="all")
    with pytest.raises(GaeHipError):
        ops.decoder_threshold_raw(torch.randn(10, 4), 0.0)
    assert ops.DecodedLinks._fields == ("indptr", "index", "score")
    links = ops.DecodedLinks(torch.tensor([0, 2, 2, 3]), torch.tensor([1, 2, 0], dtype=torch.int32), torch.zeros(3))
    row, col = links.pairs()
    assert row.dtype == col.dtype == torch.int64 and row.tolist() == [0, 0, 2] and col.tolist() == [1, 2, 0]


def test_prob_becomes_the_logit_threshold():
    from gae_dgl_amd import ops
    from gae_dgl_amd.gae import reconstruct_threshold
    assert ops.threshold_of_prob(0.5) == 0.0 and reconstruct_threshold(0.5) == 0.0 and reconstruct_threshold() == 0.0
    assert np.float32(reconstruct_threshold(0.9)) == np.float32(np.log(9.0)) == np.float32(reconstruct_threshold(0.9))
    assert reconstruct_threshold(0.9) == float(np.float32(np.log(np.float64(0.9) / (1 - np.float64(0.9)))))
    assert reconstruct_threshold(0.1) == -reconstruct_threshold(0.9)
    assert reconstruct_threshold(threshold=1.25) == 1.25
    assert reconstruct_threshold(threshold=float("-inf")) == float("-inf")


@pytest.mark.parametrize("cls", ["GAE", "VGAE"])
def test_reconstruct_refuses_bad_prob_and_both(cls):
    import gae_dgl_amd as G
    from gae_dgl_amd.vgae import VGAE
    model = G.GAE(5, [4, 3]) if cls == "GAE" else VGAE(5, [4, 3])
    g = G.DGLGraph()
    g.add_nodes(3)
    g.ndata['h'] = torch.ones(3, 5)
    for p in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="prob"):
            model.reconstruct(g, prob=p)
    with pytest.raises(ValueError, match="not both"):
        model.reconstruct(g, prob=0.5, threshold=0.0)
    with pytest.raises(ValueError, match="NaN"):
        model.reconstruct(g, threshold=float("nan"))
    assert torch.equal(g.ndata['h'], torch.ones(3, 5))     # refused before anything ran


# ------------------------------------------------------------------ metrics.reconstruction_metrics
def _csr(rows):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = [c for r in rows for c in r]
    return torch.from_numpy(indptr), torch.tensor(flat, dtype=torch.int64)


def test_reconstruction_metrics_hand_built():
    from gae_dgl_amd.metrics import reconstruction_metrics as rm
    # truth: 0 <- {1, 1, 2} (a repeat), 1 <- {0}, 2 <- {0, 2} (a self loop), 3 <- {7, -1} (outside [0, n))
    true = _csr([[1, 1, 2], [0], [0, 2], [7, -1]])
    # prediction: both entries of row 0, (1, 0), a wrong (1, 3), the self loop (2, 2), nothing else
    pred = _csr([[1, 2], [0, 3], [2], []])
    out = rm(*pred, *true)
    # positives without the diagonal: (0,1) (0,2) (1,0) (2,0): the repeat counted once, row 3 has none
    assert (out["tp"], out["fp"], out["fn"], out["n_pred"]) == (3, 1, 1, 4)
    assert out["precision"] == pytest.approx(3 / 4) and out["recall"] == pytest.approx(3 / 4)
    assert out["f1"] == pytest.approx(3 / 4) and "exact" not in out
    # with the diagonal: (2, 2) is a positive and it was predicted
    out = rm(*pred, *true, exclude_self=False)
    assert (out["tp"], out["fp"], out["fn"], out["n_pred"]) == (4, 1, 1, 5)
    assert out["precision"] == pytest.approx(4 / 5) and out["f1"] == pytest.approx(8 / 10)
    # a repeated prediction counts once too; int32 columns and numpy inputs are taken
    out = rm(np.array([0, 3, 3, 3, 3]), np.array([1, 1, 2], dtype=np.int32), *true)
    assert (out["tp"], out["fp"], out["fn"], out["n_pred"]) == (2, 0, 2, 2) and out["precision"] == 1.0


def test_reconstruction_metrics_empty_sides_give_nan():
    from gae_dgl_amd.metrics import reconstruction_metrics as rm
    true = _csr([[1], [0], []])
    none = _csr([[], [], []])
    out = rm(*none, *true)
    assert np.isnan(out["precision"]) and out["recall"] == 0.0 and out["f1"] == 0.0 and out["fn"] == 2
    out = rm(*true, *none)
    assert out["precision"] == 0.0 and np.isnan(out["recall"]) and out["f1"] == 0.0 and out["fp"] == 2
    out = rm(*none, *none, node_ptr=[0, 3])
    assert np.isnan(out["precision"]) and np.isnan(out["recall"]) and np.isnan(out["f1"])
    assert out["exact"].tolist() == [True] and out["exact_fraction"] == 1.0
    # only a diagonal on either side: empty under exclude_self
    diag = _csr([[0], [1], [2]])
    assert np.isnan(rm(*diag, *diag)["f1"]) and rm(*diag, *diag, exclude_self=False)["f1"] == 1.0
    assert np.isnan(rm(*none, *none, node_ptr=[0])["exact_fraction"])            # no member at all
    with pytest.raises(ValueError):
        rm(torch.zeros(3, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), *true)


def test_reconstruction_metrics_exact_members():
    from gae_dgl_amd.metrics import reconstruction_metrics as rm
    # two members: nodes [0, 3) a path 0 - 1 - 2, nodes [3, 5) one bond 3 - 4
    true = _csr([[1], [0, 2], [1], [4], [3]])
    pred = _csr([[1], [2, 0], [1], [4], [3, 3 + 1 - 1, 0]])         # member 1 has one extra pair: (4, 0)
    out = rm(*pred, *true, node_ptr=torch.tensor([0, 3, 5]))
    assert out["exact"].dtype == torch.bool and out["exact"].tolist() == [True, False]
    assert out["exact_fraction"] == 0.5 and (out["tp"], out["fp"], out["fn"]) == (6, 1, 0)
    # a missing pair breaks a member as an extra one does; an empty member in between is exact
    pred = _csr([[1], [0], [1], [4], [3]])
    out = rm(*pred, *true, node_ptr=[0, 3, 3, 5])
    assert out["exact"].tolist() == [False, True, True] and out["exact_fraction"] == pytest.approx(2 / 3)
    assert rm(*true, *true, node_ptr=[0, 3, 5])["exact_fraction"] == 1.0


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("extra,text", [
    (["--decode_prob", "0.5"], "need --decode_out"),
    (["--decode_max_pairs", "1000"], "need --decode_out"),
    (["--decode_out", "x.npz", "--decode_prob", "0"], "inside (0, 1)"),
    (["--decode_out", "x.npz", "--decode_prob", "1"], "inside (0, 1)"),
    (["--decode_out", "x.npz", "--decode_prob", "nan"], "inside (0, 1)"),
    (["--decode_out", "x.npz", "--decode_max_pairs", "0"], "at least 1"),
])
def test_cli_refuses_decode_combinations(extra, text, capsys, monkeypatch):
    from gae_dgl_amd import train_transductive as TT
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a device was touched"))
    with pytest.raises(SystemExit) as e:
        TT.main(["--dataset", "cora"] + extra)
    assert e.value.code == 2
    assert text in capsys.readouterr().err


def test_cli_accepts_decode():
    from gae_dgl_amd import train_transductive as TT
    a = TT.parse_args(["--decode_out", "g.npz"])
    assert a.decode_out == "g.npz" and a.decode_prob is None and a.decode_max_pairs is None
    a = TT.parse_args(["--decode_out", "g.npz", "--decode_prob", "0.9", "--decode_max_pairs", "1"])
    assert a.decode_prob == 0.9 and a.decode_max_pairs == 1
    assert TT.parse_args([]).decode_out is None
