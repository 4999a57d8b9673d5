"""CPU-side checks of the fused embedding backward (K21, gae_embed_graphs_bwd), its two host queries and the readout's
backward (gae_segment_readout_bwd): argument errors come back before any launch with a message that names the quantity,
the usable query agrees with the refusals and takes the required encoders, the workspace query is a positive function
that grows with n_out, the reference's tie rule is invisible in the weight gradients, and the command line of
gae_dgl_amd.finetune refuses bad combinations in the parser."""
import ctypes

import numpy as np
import pytest
import torch

GAE_OK, GAE_E_NULL, GAE_E_SIZE, GAE_E_DTYPE, GAE_E_RANGE = 0, -1, -2, -4, -6
F32, U8 = 0, 2
FAKE = 0x10000          # a non-NULL "device pointer": the checks below must return before anything is dereferenced

REQUIRED = [(39, (32, 16)), (39, (16,)), (39, (64, 32, 16)), (39, (32, 32, 32, 8))]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def ws_bytes(lib, f_in, widths, n_out):
    arr = (ctypes.c_int64 * max(len(widths), 1))(*widths)
    return lib.gae_embed_graphs_bwd_workspace_bytes(f_in, len(widths), arr, n_out)


def call(lib, *, widths=(32, 16), f_in=39, acts=None, norm=0, ldd=None, n_graphs=8, n_nodes=100, n_edges=200,
         max_nodes=38, n_out=0, dtype=U8, ldf=48, ldw=None, lddw=None, null=(), weight_null=None, want=False, ws=None,
         ws_size=0, arrays=(FAKE, FAKE, FAKE, FAKE), d_out=FAKE):
    """gae_embed_graphs_bwd with valid arguments except the ones overridden.  n_out = 0 and no gradient wanted by
    default: a valid call that launches nothing and needs no GPU"""
    L = len(widths)
    c_widths = (ctypes.c_int64 * L)(*widths)
    c_w = (ctypes.c_void_p * L)(*[FAKE] * L)
    if weight_null is not None:
        c_w[weight_null] = None
    ins = [f_in] + list(widths[:-1])
    c_ldw = (ctypes.c_int64 * L)(*(ldw if ldw is not None else ins))
    c_lddw = (ctypes.c_int64 * L)(*(lddw if lddw is not None else ins))
    c_b = (ctypes.c_void_p * L)(*[FAKE] * L)
    c_acts = (ctypes.c_int * L)(*(acts if acts is not None else [1] * (L - 1) + [0]))
    c_dw = (ctypes.c_void_p * L)(*[FAKE if want else None] * L)
    c_db = (ctypes.c_void_p * L)(*[FAKE if want else None] * L)
    arg = {"widths": c_widths, "weights": c_w, "ldw": c_ldw, "acts": c_acts, "dW": c_dw, "lddw": c_lddw, "db": c_db}
    for k in null:
        arg[k] = None
    gp, ip, ix, feat = arrays
    rc = lib.gae_embed_graphs_bwd(gp, n_graphs, n_nodes, n_edges, max_nodes, ip, ix, feat, dtype, ldf, f_in, L,
                                  arg["widths"], arg["weights"], arg["ldw"], c_b, arg["acts"], norm, None, n_out, d_out,
                                  3 * widths[-1] if ldd is None else ldd, arg["dW"], arg["lddw"], arg["db"], ws, ws_size,
                                  None)
    return rc, lib.gae_last_error().decode()


def test_a_valid_request_for_no_output_is_ok_without_a_gpu(lib):
    for f_in, widths in REQUIRED:
        assert call(lib, f_in=f_in, widths=widths, max_nodes=64)[0] == GAE_OK
    assert call(lib, dtype=F32, ldf=40)[0] == GAE_OK
    assert call(lib, n_out=8)[0] == GAE_OK          # no gradient wanted: nothing to do, nothing launched


@pytest.mark.parametrize("name", ["widths", "weights", "ldw", "acts", "dW", "lddw", "db"])
def test_null_tables_are_refused(lib, name):
    rc, msg = call(lib, null=(name,))
    assert rc == GAE_E_NULL and "NULL" in msg and "gae_embed_graphs_bwd" in msg
    if name in ("dW", "lddw", "db"):
        assert "dW / lddw / db" in msg


def test_null_weight_of_a_layer_names_the_layer(lib):
    rc, msg = call(lib, weight_null=1)
    assert rc == GAE_E_NULL and "layer 1" in msg


@pytest.mark.parametrize("kw,word", [({"n_graphs": -1}, "n_graphs = -1"), ({"n_nodes": -5}, "n_nodes = -5"),
                                     ({"n_edges": -2}, "n_edges = -2"), ({"n_out": -3}, "n_out = -3"),
                                     ({"max_nodes": -1}, "max_graph_nodes = -1")])
def test_negative_sizes_name_the_quantity(lib, kw, word):
    rc, msg = call(lib, **kw)
    assert rc == GAE_E_SIZE and "negative" in msg and word in msg


def test_leading_dimensions_and_feature_rows(lib):
    rc, msg = call(lib, ldd=47)
    assert rc == GAE_E_SIZE and "ldd 47 < 3 d = 48" in msg
    assert call(lib, ldd=48)[0] == GAE_OK and call(lib, ldd=64)[0] == GAE_OK
    rc, msg = call(lib, ldw=(38, 32))
    assert rc == GAE_E_SIZE and "ldw = 38" in msg and "layer 0" in msg
    rc, msg = call(lib, lddw=(39, 31), want=True)
    assert rc == GAE_E_SIZE and "lddw = 31" in msg and "layer 1" in msg
    rc, msg = call(lib, ldf=39)
    assert rc == GAE_E_SIZE and "ldf = 39" in msg
    rc, msg = call(lib, norm=2)
    assert rc == GAE_E_RANGE and "norm code 2" in msg
    rc, msg = call(lib, dtype=1)
    assert rc == GAE_E_DTYPE and "dtype 1" in msg
    rc, msg = call(lib, acts=(1, 7))
    assert rc == GAE_E_DTYPE and "activation code 7" in msg and "layer 1" in msg


def test_a_workspace_that_is_missing_or_too_small_is_refused_before_any_launch(lib):
    need = ws_bytes(lib, 39, (32, 16), 8)
    assert need > 0
    rc, msg = call(lib, n_out=8, want=True, ws=None, ws_size=need)
    assert rc == GAE_E_SIZE and "workspace" in msg and str(need) in msg
    rc, msg = call(lib, n_out=8, want=True, ws=FAKE, ws_size=need - 1)
    assert rc == GAE_E_SIZE and f"workspace of {need - 1} bytes, {need} needed" in msg
    # a large enough workspace: the next check (NULL arrays) answers, still before any launch
    for arrays, d_out, word in (((None, FAKE, FAKE, FAKE), FAKE, "graph_ptr"), ((FAKE, FAKE, FAKE, FAKE), None, "d_out"),
                                ((FAKE, None, FAKE, FAKE), FAKE, "indptr"), ((FAKE, FAKE, FAKE, None), FAKE, "feat"),
                                ((FAKE, FAKE, None, FAKE), FAKE, "indices")):
        rc, msg = call(lib, n_out=8, want=True, ws=FAKE, ws_size=need, arrays=arrays, d_out=d_out)
        assert rc == GAE_E_NULL and word in msg, (word, msg)


SHAPES = [(39, (32, 16), 64, True), (39, (16,), 64, True), (39, (64, 32, 16), 64, True), (39, (32, 32, 32, 8), 64, True),
          (39, (32, 16), 38, True), (1, (1,), 1, True), (64, (64,), 64, True), (39, (64, 64), 64, True),
          (64, (64, 64, 64, 64), 64, False),          # the forward's full envelope: LDS and accumulator tiles
          (39, (64, 64, 64), 64, False),              # 10 tiles of 32 x 32
          (39, (32, 16), 65, False), (65, (16,), 10, False), (39, (65,), 10, False), (39, (), 10, False),
          (39, (8, 8, 8, 8, 8), 10, False), (0, (16,), 10, False), (39, (16, 0), 10, False)]


@pytest.mark.parametrize("f_in,widths,max_nodes,taken", SHAPES)
def test_usable_agrees_with_the_refusals(lib, f_in, widths, max_nodes, taken):
    from gae_dgl_amd import ops
    arr = (ctypes.c_int64 * max(len(widths), 1))(*widths)
    assert lib.gae_embed_graphs_bwd_usable(f_in, len(widths), arr, max_nodes) == int(taken)
    assert ops.embed_graphs_bwd_usable(f_in, widths, max_nodes) is taken
    if taken:
        assert ops.embed_graphs_usable(f_in, widths, max_nodes)              # never wider than the forward
    if len(widths) == 0:
        return
    dtype, ldf = (F32, (f_in + 3) // 4 * 4) if f_in > 0 else (F32, 4)
    rc, msg = call(lib, f_in=f_in, widths=widths, max_nodes=max_nodes, dtype=dtype, ldf=ldf)
    assert (rc == GAE_OK) is taken, msg
    if not taken:
        assert rc == GAE_E_RANGE and "gae_embed_graphs_bwd" in msg
        assert any(w in msg for w in ("n_layers", "f_in", "width of layer", "max_graph_nodes", "tiles", "LDS")), msg
    if max_nodes <= 64:
        assert (ws_bytes(lib, f_in, widths, 100) > 0) is taken


def test_usable_refuses_null_widths_and_negative_bounds(lib):
    assert lib.gae_embed_graphs_bwd_usable(39, 2, None, 38) == 0
    assert lib.gae_embed_graphs_bwd_usable(39, 2, (ctypes.c_int64 * 2)(32, 16), -1) == 0
    assert lib.gae_embed_graphs_bwd_workspace_bytes(39, 2, None, 10) == GAE_E_NULL
    assert ws_bytes(lib, 39, (32, 16), -1) == GAE_E_SIZE and "n_out = -1" in lib.gae_last_error().decode()


@pytest.mark.parametrize("f_in,widths", REQUIRED)
def test_workspace_bytes_is_positive_and_grows_with_n_out(lib, f_in, widths):
    ns = [0, 1, 3, 4, 5, 127, 128, 1000, 1024, 1025, 4096, 8192, 8193, 10000, 16384, 16385, 100000, 131072, 131073,
          249455, 1000000]
    got = [ws_bytes(lib, f_in, widths, n) for n in ns]
    assert all(g > 0 for g in got)
    assert all(a <= b for a, b in zip(got, got[1:])), got
    params = sum(o * i + o for i, o in zip((f_in,) + widths[:-1], widths))
    assert all(g % (4 * params) == 0 for g in got)              # whole partials: one value per parameter


def test_readout_bwd_argument_errors(lib):
    rc = lib.gae_segment_readout_bwd(FAKE, 16, -1, 16, FAKE, 4, FAKE, 48, FAKE, 16, None)
    assert rc == GAE_E_SIZE and "n_nodes = -1" in lib.gae_last_error().decode()
    rc = lib.gae_segment_readout_bwd(FAKE, 16, 10, 16, FAKE, 4, FAKE, 47, FAKE, 16, None)
    assert rc == GAE_E_SIZE and "ldd 47 < 3 d = 48" in lib.gae_last_error().decode()
    rc = lib.gae_segment_readout_bwd(FAKE, 15, 10, 16, FAKE, 4, FAKE, 48, FAKE, 16, None)
    assert rc == GAE_E_SIZE and "ldz 15" in lib.gae_last_error().decode()
    rc = lib.gae_segment_readout_bwd(FAKE, 16, 10, 16, FAKE, 4, FAKE, 48, FAKE, 15, None)
    assert rc == GAE_E_SIZE and "lddz 15" in lib.gae_last_error().decode()
    for args in ((None, 16, 10, 16, FAKE, 4, FAKE, 48, FAKE, 16), (FAKE, 16, 10, 16, None, 4, FAKE, 48, FAKE, 16),
                 (FAKE, 16, 10, 16, FAKE, 4, None, 48, FAKE, 16), (FAKE, 16, 10, 16, FAKE, 4, FAKE, 48, None, 16)):
        assert lib.gae_segment_readout_bwd(*args, None) == GAE_E_NULL and "NULL" in lib.gae_last_error().decode()
    assert lib.gae_segment_readout_bwd(None, 16, 0, 16, FAKE, 4, None, 48, None, 16, None) == GAE_OK     # no rows
    assert lib.gae_segment_readout_bwd(None, 16, 10, 16, None, 0, None, 48, None, 16, None) == GAE_OK    # no graphs


def test_wrappers_refuse_cpu_tensors():
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    gp = torch.tensor([0, 2]); ip = torch.tensor([0, 1, 2], dtype=torch.int32); ix = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(GaeHipError):
        ops.embed_graphs_bwd(gp, ip, ix, torch.zeros(2, 4), [torch.zeros(3, 4)], [None], [0], torch.zeros(1, 9))
    with pytest.raises(GaeHipError):
        ops.segment_readout_bwd(torch.zeros(2, 3), gp, torch.zeros(1, 9))
    import gae_dgl_amd as G
    with pytest.raises(ValueError, match="grad"):
        G.GAE(39, [32, 16]).embed_graphs(None, grad="yes")


# ------------------------------------------------------------------ the reference itself
def test_reference_readout_and_its_tie_rules():
    """the restated readout equals oracle.segment_readout; on duplicated rows the whole d_max lands on the first (last)
    row attaining the maximum; mean and sum spread evenly"""
    import embed_grad_ref as R
    rng = np.random.default_rng(0)
    Z = rng.standard_normal((9, 3))
    Z[4] = Z[2]; Z[5] = Z[2]                                       # graph 1 = rows 2..5: three equal rows
    gp = np.array([0, 2, 6, 6, 9])
    got = R.readout(torch.from_numpy(Z), gp)
    assert np.allclose(got.numpy(), R.O().segment_readout(Z, gp), atol=1e-15)
    d_out = np.zeros((4, 9)); d_out[:, 6:] = 1.0                  # d_max only
    first, last = R.readout_dz(Z, gp, d_out, "first").numpy(), R.readout_dz(Z, gp, d_out, "last").numpy()
    for c in range(3):
        top = np.nonzero(Z[2:6, c] == Z[2:6, c].max())[0] + 2
        assert first[2:6, c].sum() == 1.0 and first[top[0], c] == 1.0
        assert last[2:6, c].sum() == 1.0 and last[top[-1], c] == 1.0
    d_out = rng.standard_normal((4, 9)); d_out[:, 6:] = 0.0
    dz = R.readout_dz(Z, gp, d_out).numpy()
    assert np.allclose(dz[2:6], d_out[1, 3:6] + d_out[1, :3] / 4)


@pytest.mark.parametrize("norm", ["none", "both"])
def test_the_tie_rule_is_invisible_in_the_weight_gradients(norm):
    """the precondition of the GPU comparison, here on 60 ZINC-like molecules (symmetric atoms tie exactly): first-row
    and last-row gradients agree to 1e-9 -- encoder_grads asserts it on every input it is given"""
    import embed_grad_ref as R
    import gae_dgl_amd as G
    from gae_dgl_amd import workloads
    gp, src, dst, X = workloads.zinc_like(60, seed=7)
    torch.manual_seed(1)
    model = G.GAE(39, [32, 16])
    d_out = torch.randn(60, 48, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    F, dWs, dbs = R.encoder_grads(gp, src, dst, X, model, norm, d_out)
    assert F.shape == (60, 48) and [tuple(w.shape) for w in dWs] == [(32, 39), (16, 32)]
    assert all(float(g.abs().max()) > 0 for g in dWs + dbs)
    # a list with a repeat contributes twice
    F2, dW2, _ = R.encoder_grads(gp, src, dst, X, model, norm, d_out[:3], graph_ids=[5, 1, 5])
    only5 = R.encoder_grads(gp, src, dst, X, model, norm, d_out[0:1] + d_out[2:3], graph_ids=[5])[1]
    only1 = R.encoder_grads(gp, src, dst, X, model, norm, d_out[1:2], graph_ids=[1])[1]
    assert R.rel_err(dW2[0], only5[0] + only1[0]) < 1e-12 and torch.equal(F2[0], F2[2])


# ------------------------------------------------------------------ the command line
def test_finetune_parser_refuses_bad_combinations(capsys):
    from gae_dgl_amd import finetune as FT
    ok = ["--checkpoint", "ep09.pkl", "--hidden_dims", "32", "16", "-d", "graphs.npz", "--targets", "y.npy", "--out", "o"]
    args = FT.parse_args(ok + ["--head", "mlp", "--freeze_encoder", "--epochs", "3", "-b", "128", "--lr", "0.01"])
    assert args.head == "mlp" and args.freeze_encoder and args.epochs == 3 and args.batch_size == 128 and args.lr == 0.01
    assert FT.parse_args(ok).head == "linear" and FT.parse_args(ok).fused == "auto"

    def refused(argv, word):
        with pytest.raises(SystemExit):
            FT.parse_args(argv)
        assert word in capsys.readouterr().err

    refused(ok[2:], "--checkpoint")
    refused(ok[:2] + ok[5:], "--hidden_dims")
    refused(ok[:7] + ok[9:], "--targets")
    refused(ok[:9], "--out")
    refused(ok[:5] + ok[7:], "exactly one of")
    refused(ok + ["--synthetic", "100"], "exactly one of")
    refused(ok + ["--epochs", "0"], "positive")
    refused(ok + ["-b", "0"], "positive")
    refused(ok + ["--lr", "0"], "--lr")
    refused(ok + ["--head", "forest"], "invalid choice")
    refused(ok[:2] + ["--hidden_dims", "64", "64", "64", "64", "-i", "64"] + ok[5:] + ["--fused", "on"], "--fused on")
    FT.parse_args(ok[:2] + ["--hidden_dims", "64", "64", "64", "64", "-i", "64"] + ok[5:] + ["--fused", "on",
                                                                                          "--freeze_encoder"])
