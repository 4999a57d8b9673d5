"""CPU-side checks of the per-graph reconstruction scores (K20, gae_score_graphs): the numpy reference of the GPU tests
agrees with metrics.roc_auc / metrics.average_precision; every argument error of the entry point is reported before any
launch; the usable-queries of K19 and K20 agree; graph_score_summary on hand-made counts; the band fixture of the GPU
tests is tight enough to say something, judged by the oracle alone."""
import ctypes

import numpy as np
import pytest
import torch

import score_ref as R

GAE_OK, GAE_E_NULL, GAE_E_SIZE, GAE_E_DTYPE, GAE_E_RANGE = 0, -1, -2, -4, -6
F32, U8 = 0, 2
FAKE = 0x10000          # a non-NULL "device pointer": the checks below must return before anything is dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


# ------------------------------------------------------------------ the reference against metrics.py
def _random_graph(rng, n, ties, repeats):
    e = int(rng.integers(1, 3 * n + 2))
    rows, cols = rng.integers(0, n, e), rng.integers(0, n, e)
    if repeats and e > 3:
        rows[:2], cols[:2] = rows[2:4], cols[2:4]
    indptr, indices = R.csr_rows(n, rows, cols)
    d = int(rng.integers(1, 9))
    Z = rng.integers(-2, 3, (n, d)).astype(np.float64) if ties else rng.standard_normal((n, d))
    return Z, indptr, indices


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("exclude_self", [True, False])
def test_reference_agrees_with_roc_auc_and_average_precision(ties, exclude_self):
    from gae_dgl_amd import metrics
    rng = np.random.default_rng(3 + ties)
    checked = 0
    for trial in range(40):
        n = int(rng.integers(2, 20))
        Z, indptr, indices = _random_graph(rng, n, ties, repeats=trial % 2 == 0)
        r = R.graph_scores(Z, indptr, indices, 0, n, exclude_self)
        assert r["n_pos"] + r["n_neg"] == n * n - (n if exclude_self else 0)
        if r["n_pos"] == 0 or r["n_neg"] == 0:
            assert np.isnan(r["auc"]) and np.isnan(r["ap"])
            continue
        P, Q = torch.from_numpy(r["pos"]), torch.from_numpy(r["neg"])
        assert abs(r["auc"] - metrics.roc_auc(P, Q)) < 1e-12
        assert abs(r["ap"] - metrics.average_precision(P, Q)) < 1e-12
        if ties:
            assert r["ties"] > 0 or n < 4
        checked += 1
    assert checked >= 30


def test_reference_counts_a_repeated_entry_once_and_ignores_foreign_columns():
    # graph of rows [2, 5) inside a 6-row CSR: row 2 lists column 3 twice, column 0 (foreign) and itself
    indptr, indices = R.csr_rows(6, [2, 2, 2, 2, 4], [3, 3, 0, 2, 3])
    Z = np.array([[9.0], [9.0], [1.0], [2.0], [3.0], [9.0]])
    r = R.graph_scores(Z, indptr, indices, 2, 3, True)
    assert (r["n_pos"], r["n_neg"]) == (2, 4) and list(r["pos"]) == [2.0, 6.0]
    assert sorted(r["neg"]) == [2.0, 3.0, 3.0, 6.0] and (r["wins"], r["ties"]) == (3, 2)
    r = R.graph_scores(Z, indptr, indices, 2, 3, False)
    assert (r["n_pos"], r["n_neg"]) == (3, 6) and list(r["pos"]) == [2.0, 1.0, 6.0]
    # the loss sees the repeat and the self loop: S = 4 entries inside the graph
    s = Z[2:5] @ Z[2:5].T
    y = np.zeros((3, 3)); y[0, 1] = 2; y[0, 0] = 1; y[2, 1] = 1
    pw = (9 - 4) / 4
    sp = lambda v: np.logaddexp(0, v)      # noqa: E731
    assert abs(r["loss"] - float((sp(s) + y * ((pw - 1) * sp(-s) - s)).sum() / 9)) < 1e-12


def test_dense_routine_follows_the_reference():
    from gae_dgl_amd import metrics
    rng = np.random.default_rng(8)
    for trial in range(12):
        n = int(rng.integers(1, 30))
        Z, indptr, indices = _random_graph(rng, n, ties=trial % 2 == 0, repeats=True)
        Z = Z.astype(np.float32)
        for ex in (True, False):
            r = R.graph_scores(Z, indptr, indices, 0, n, ex)
            m = metrics.graph_scores_dense(torch.from_numpy(Z), (torch.from_numpy(indptr), torch.from_numpy(indices)), ex)
            if trial % 2 == 0:                                        # integer logits: exact
                assert [m[k] for k in ("n_pos", "n_neg", "wins", "ties")] == [r[k] for k in ("n_pos", "n_neg", "wins", "ties")]
            for k in ("auc", "ap", "loss"):
                if trial % 2 == 0 or k == "loss":
                    assert (np.isnan(m[k]) and np.isnan(r[k])) or abs(m[k] - r[k]) <= 1e-5 * max(1, abs(r[k])), (k, m[k], r[k])
    bad = metrics.graph_scores_dense(torch.tensor([[float("inf")], [1.0]]), (torch.tensor([0, 1, 1]), torch.tensor([1])))
    assert bad["n_pos"] == -1 and np.isnan(bad["loss"])


# ------------------------------------------------------------------ argument errors without a GPU
def call(lib, *, widths=(32, 16), f_in=39, acts=None, norm=0, n_graphs=8, n_nodes=100, n_edges=200, max_nodes=38,
         n_out=0, dtype=U8, ldf=48, ldw=None, null=(), n_layers=None, weight_null=None, exclude_self=1, outs=(FAKE,) * 3,
         graph_ptr=FAKE, indptr=FAKE, indices=FAKE, feat=FAKE):
    """gae_score_graphs with valid arguments except the ones overridden; n_out = 0 by default: a valid call launches
    nothing (and needs no GPU)"""
    L = len(widths) if n_layers is None else n_layers
    n = max(len(widths), 1)
    c_widths = (ctypes.c_int64 * n)(*widths)
    c_w = (ctypes.c_void_p * n)(*[FAKE] * n)
    if weight_null is not None:
        c_w[weight_null] = None
    ins = [f_in] + list(widths[:-1])
    c_ldw = (ctypes.c_int64 * n)(*(ldw if ldw is not None else ins[:n]))
    c_b = (ctypes.c_void_p * n)(*[FAKE] * n)
    c_acts = (ctypes.c_int * n)(*(acts if acts is not None else [1] * (len(widths) - 1) + [0] * min(len(widths), 1)))
    arg = {"widths": c_widths, "weights": c_w, "ldw": c_ldw, "acts": c_acts}
    for k in null:
        arg[k] = None
    rc = lib.gae_score_graphs(graph_ptr, n_graphs, n_nodes, n_edges, max_nodes, indptr, indices, feat, dtype, ldf, f_in, L,
                              arg["widths"], arg["weights"], arg["ldw"], c_b, arg["acts"], norm, None, n_out,
                              exclude_self, outs[0], outs[1], outs[2], None)
    return rc, lib.gae_last_error().decode()


def test_a_valid_request_for_no_output_is_ok_without_a_gpu(lib):
    assert call(lib)[0] == GAE_OK
    assert call(lib, widths=(64, 64, 64, 64), f_in=64, dtype=F32, ldf=64, max_nodes=64)[0] == GAE_OK
    assert call(lib, exclude_self=0)[0] == GAE_OK
    # no layers: the fp32 rows are Z; the layer tables may be NULL
    assert call(lib, widths=(), f_in=16, dtype=F32, ldf=16, null=("widths", "weights", "ldw", "acts"))[0] == GAE_OK
    assert call(lib, widths=(), f_in=1, dtype=F32, ldf=4)[0] == GAE_OK


@pytest.mark.parametrize("name", ["widths", "weights", "ldw", "acts"])
def test_null_layer_tables_are_refused_when_there_are_layers(lib, name):
    rc, msg = call(lib, null=(name,))
    assert rc == GAE_E_NULL and "NULL" in msg and "gae_score_graphs" in msg


def test_argument_errors_name_the_quantity(lib):
    rc, msg = call(lib, weight_null=1)
    assert rc == GAE_E_NULL and "layer 1" in msg
    for kw, word in (({"n_graphs": -1}, "n_graphs = -1"), ({"n_nodes": -5}, "n_nodes = -5"), ({"n_edges": -2}, "n_edges = -2"),
                     ({"n_out": -3}, "n_out = -3"), ({"max_nodes": -1}, "max_graph_nodes = -1")):
        rc, msg = call(lib, **kw)
        assert rc == GAE_E_SIZE and "negative" in msg and word in msg and "gae_score_graphs" in msg
    rc, msg = call(lib, widths=(32, 32, 32, 32, 16))
    assert rc == GAE_E_RANGE and "n_layers = 5" in msg and "0..4" in msg
    rc, msg = call(lib, widths=(65, 16))
    assert rc == GAE_E_RANGE and "layer 0" in msg and "65" in msg
    rc, msg = call(lib, widths=(), f_in=65, dtype=F32, ldf=68)
    assert rc == GAE_E_RANGE and "f_in = 65" in msg
    rc, msg = call(lib, max_nodes=65)
    assert rc == GAE_E_RANGE and "max_graph_nodes = 65" in msg
    rc, msg = call(lib, ldw=(38, 32))
    assert rc == GAE_E_SIZE and "ldw = 38" in msg and "layer 0" in msg
    rc, msg = call(lib, ldf=39)
    assert rc == GAE_E_SIZE and "ldf = 39" in msg
    rc, msg = call(lib, norm=2)
    assert rc == GAE_E_RANGE and "norm code 2" in msg
    rc, msg = call(lib, acts=(1, 7))
    assert rc == GAE_E_DTYPE and "activation code 7" in msg and "layer 1" in msg
    rc, msg = call(lib, dtype=1)
    assert rc == GAE_E_DTYPE and "dtype 1" in msg
    rc, msg = call(lib, exclude_self=2)
    assert rc == GAE_E_RANGE and "exclude_self = 2" in msg
    rc, msg = call(lib, widths=(), f_in=16, dtype=U8, ldf=16)
    assert rc == GAE_E_DTYPE and "n_layers = 0" in msg


def test_null_arrays_are_refused_when_there_is_output(lib):
    for kw, word in (({"graph_ptr": None}, "graph_ptr"), ({"indptr": None}, "indptr"), ({"feat": None}, "feat"),
                     ({"indices": None}, "indices"), ({"outs": (None, FAKE, FAKE)}, "counts_out"),
                     ({"outs": (FAKE, None, FAKE)}, "ap_out"), ({"outs": (FAKE, FAKE, None)}, "loss_out")):
        rc, msg = call(lib, n_out=8, **kw)
        assert rc == GAE_E_NULL and word in msg, (word, msg)


SHAPES = [  # f_in, widths, max nodes, taken by K19?, taken by K20?
    (39, (32, 16), 38, True, True), (39, (16,), 64, True, True), (64, (64, 64, 64, 64), 64, True, True),
    (1, (1,), 1, True, True), (39, (32, 32, 32, 32, 16), 38, False, False), (39, (128, 64), 38, False, False),
    (65, (32, 16), 38, False, False), (39, (32, 0), 38, False, False), (39, (32, 16), 65, False, False),
    (16, (), 38, False, True), (64, (), 64, False, True), (1, (), 0, False, True), (65, (), 38, False, False),
    (0, (), 38, False, False), (16, (), 65, False, False),
]


@pytest.mark.parametrize("f_in,widths,max_nodes,k19,k20", SHAPES)
def test_usable_queries_agree_with_each_other_and_with_the_refusals(lib, f_in, widths, max_nodes, k19, k20):
    from gae_dgl_amd import ops
    assert ops.embed_graphs_usable(f_in, widths, max_nodes) is k19
    assert ops.score_graphs_usable(f_in, widths, max_nodes) is k20
    if widths:
        assert k19 == k20                                                  # one answer for n_layers >= 1
    rc, msg = call(lib, widths=widths, f_in=f_in, max_nodes=max_nodes, dtype=F32, ldf=(max(f_in, 1) + 3) // 4 * 4)
    assert (rc == GAE_OK) is k20, msg
    if not k20:
        assert rc == GAE_E_RANGE and ("outside" in msg or "above" in msg)
    assert lib.gae_score_graphs_usable(39, 2, None, 38) == 0               # layers without widths: never usable
    assert lib.gae_score_graphs_usable(16, 0, None, 38) == 1
    assert lib.gae_score_graphs_usable(16, 0, None, -1) == 0


def test_wrapper_and_model_check_their_arguments_without_a_gpu():
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    gp = torch.tensor([0, 2], dtype=torch.int64)
    ip = torch.tensor([0, 1, 2], dtype=torch.int32)
    ix = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(GaeHipError, match="no CPU fallback"):
        ops.score_graphs(gp, ip, ix, torch.zeros(2, 4))
    m = G.GAE(39, [32, 16])
    with pytest.raises(ValueError, match="fused"):
        m.score_graphs(None, fused="yes")
    with pytest.raises(ValueError, match="batch_size"):
        m.score_graphs(None, batch_size=0)
    assert ops.GraphScores._fields == ("loss", "auc", "ap", "n_pos", "n_neg", "wins", "ties")
    from gae_dgl_amd.vgae import VGAE
    assert hasattr(VGAE, "score_graphs")


# ------------------------------------------------------------------ the summary
def test_summary_of_hand_made_counts():
    from gae_dgl_amd import metrics, ops
    nan = float("nan")
    s = ops.GraphScores(loss=torch.tensor([1.0, 3.0, nan, nan, 2.0]),
                        auc=torch.tensor([1.0, 0.5, nan, nan, nan], dtype=torch.float64),
                        ap=torch.tensor([1.0, 0.25, nan, nan, nan], dtype=torch.float64),
                        n_pos=torch.tensor([2, 4, 0, -1, 6]), n_neg=torch.tensor([4, 8, 6, -1, 0]),
                        wins=torch.tensor([8, 12, 0, -1, 0]), ties=torch.tensor([0, 8, 0, -1, 0]))
    out = metrics.graph_score_summary(s)
    assert out["graphs"] == 2 and out["left_out"] == 3
    assert out["auc"] == 0.75 and out["ap"] == 0.625 and out["loss"] == 2.0
    assert out["micro_auc"] == (8 + 12 + 8 / 2) / (2 * 4 + 4 * 8)
    empty = metrics.graph_score_summary(ops.GraphScores(*(torch.zeros(0) for _ in range(7))))
    assert empty["graphs"] == 0 and empty["left_out"] == 0 and all(np.isnan(empty[k]) for k in ("auc", "ap", "loss", "micro_auc"))
    none = metrics.graph_score_summary(ops.GraphScores(torch.tensor([nan]), torch.tensor([nan]), torch.tensor([nan]),
                                                       torch.tensor([0]), torch.tensor([0]), torch.tensor([0]), torch.tensor([0])))
    assert none["graphs"] == 0 and none["left_out"] == 1 and np.isnan(none["micro_auc"])


# ------------------------------------------------------------------ the fixtures of the GPU tests, by the oracle alone
@pytest.mark.parametrize("norm", ["none", "both"])
def test_band_fixture_leaves_less_than_one_percent_open(norm):
    """item 3 of the GPU tests bounds wins from below by lo and wins + ties from above by hi; that says something only
    if few (positive, negative) pairs lie within 2 delta of each other: hi - lo <= 1 % of all pairs over the fixture"""
    gp, rows, cols, X, Ws, bs = R.band_fixture()
    indptr, indices = R.csr_rows(int(gp[-1]), rows, cols)
    _, logits = R.set_scores(gp, indptr, indices, X, Ws, bs, norm)
    bands, delta, open_pairs, pairs = R.band_totals(gp, indptr, indices, logits)
    print(f"band fixture norm={norm}: delta {delta:.3e}, open {open_pairs} of {pairs} pairs = {open_pairs / pairs:.3e}")
    assert pairs > 1e6 and open_pairs <= 0.01 * pairs
    for b in bands:
        assert b["lo"] <= b["wins"] and b["wins"] + b["ties"] <= b["hi"]
        assert b["ap_lo"] - 1e-12 <= b["ap"] <= b["ap_hi"] + 1e-12         # (a mean against a chain: rounding)


@pytest.mark.parametrize("hidden", [[8, 4], [16, 8, 4]], ids=lambda h: "x".join(map(str, h)))
def test_integer_encoder_fixture_stays_below_two_to_the_24(hidden):
    gp, rows, cols, X, Ws, bs = R.integer_fixture(hidden)
    indptr, indices = R.csr_rows(int(gp[-1]), rows, cols)
    scores, logits = R.set_scores(gp, indptr, indices, X, Ws, bs, "none", integers=True)      # asserts the bound
    assert sum(r["ties"] for r in scores) > 1000                          # ties are plentiful: that is the point
    assert any(np.abs(s).max() > 0 for s in logits)

