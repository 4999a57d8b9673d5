"""CPU-side checks of the fused embedding entry points (K19, gae_embed_graphs): every argument error is reported before
any launch, with a message that names the quantity; the usable-query agrees with the refusals; the command line of
gae_dgl_amd.embed refuses bad combinations in the parser."""
import ctypes

import pytest

GAE_OK, GAE_E_NULL, GAE_E_SIZE, GAE_E_DTYPE, GAE_E_RANGE = 0, -1, -2, -4, -6
F32, U8 = 0, 2
FAKE = 0x10000          # a non-NULL "device pointer": the checks below must return before anything is dereferenced


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def call(lib, *, widths=(32, 16), f_in=39, acts=None, norm=0, ldo=None, n_graphs=8, n_nodes=100, n_edges=200,
         max_nodes=38, n_out=0, dtype=U8, ldf=48, ldw=None, null=(), n_layers=None, weight_null=None):
    """gae_embed_graphs with valid arguments except the ones overridden; n_out = 0 by default: a valid call launches
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
    c_acts = (ctypes.c_int * n)(*(acts if acts is not None else [1] * (len(widths) - 1) + [0]))
    d = widths[-1] if widths else 1
    arg = {"widths": c_widths, "weights": c_w, "ldw": c_ldw, "acts": c_acts}
    for k in null:
        arg[k] = None
    rc = lib.gae_embed_graphs(FAKE, n_graphs, n_nodes, n_edges, max_nodes, FAKE, FAKE, FAKE, dtype, ldf, f_in, L,
                              arg["widths"], arg["weights"], arg["ldw"], c_b, arg["acts"], norm, None, n_out, FAKE,
                              3 * d if ldo is None else ldo, None)
    return rc, lib.gae_last_error().decode()


def test_a_valid_request_for_no_output_is_ok_without_a_gpu(lib):
    assert call(lib)[0] == GAE_OK
    assert call(lib, widths=(16,))[0] == GAE_OK
    assert call(lib, widths=(64, 64, 64, 64), f_in=64, dtype=F32, ldf=64, max_nodes=64)[0] == GAE_OK


@pytest.mark.parametrize("name", ["widths", "weights", "ldw", "acts"])
def test_null_layer_tables_are_refused(lib, name):
    rc, msg = call(lib, null=(name,))
    assert rc == GAE_E_NULL and "NULL" in msg and "gae_embed_graphs" in msg


def test_null_weight_of_a_layer_names_the_layer(lib):
    rc, msg = call(lib, weight_null=1)
    assert rc == GAE_E_NULL and "layer 1" in msg


def test_null_arrays_are_refused_when_there_is_output(lib):
    L = 2
    w = (ctypes.c_int64 * L)(32, 16)
    wp = (ctypes.c_void_p * L)(FAKE, FAKE)
    ldw = (ctypes.c_int64 * L)(39, 32)
    acts = (ctypes.c_int * L)(1, 0)
    # graph_ptr NULL, then out NULL, then indptr / feat NULL, then indices NULL
    for args, word in (((None, 8, 100, 200, 38, FAKE, FAKE, FAKE), "graph_ptr"),
                       ((FAKE, 8, 100, 200, 38, None, FAKE, FAKE), "indptr"),
                       ((FAKE, 8, 100, 200, 38, FAKE, FAKE, None), "feat"),
                       ((FAKE, 8, 100, 200, 38, FAKE, None, FAKE), "indices")):
        rc = lib.gae_embed_graphs(*args, U8, 48, 39, L, w, wp, ldw, None, acts, 0, None, 8, FAKE, 48, None)
        assert rc == GAE_E_NULL and word in lib.gae_last_error().decode(), (word, lib.gae_last_error())
    rc = lib.gae_embed_graphs(FAKE, 8, 100, 200, 38, FAKE, FAKE, FAKE, U8, 48, 39, L, w, wp, ldw, None, acts, 0, None, 8,
                              None, 48, None)
    assert rc == GAE_E_NULL and "out" in lib.gae_last_error().decode()


@pytest.mark.parametrize("kw,word", [({"n_graphs": -1}, "n_graphs = -1"), ({"n_nodes": -5}, "n_nodes = -5"),
                                      ({"n_edges": -2}, "n_edges = -2"), ({"n_out": -3}, "n_out = -3"),
                                      ({"max_nodes": -1}, "max_graph_nodes = -1")])
def test_negative_sizes_are_refused(lib, kw, word):
    rc, msg = call(lib, **kw)
    assert rc == GAE_E_SIZE and "negative" in msg and word in msg


def test_layer_count_outside_1_to_4_is_refused(lib):
    rc, msg = call(lib, widths=(), n_layers=0)
    assert rc == GAE_E_RANGE and "n_layers = 0" in msg
    rc, msg = call(lib, widths=(32, 32, 32, 32, 16))
    assert rc == GAE_E_RANGE and "n_layers = 5" in msg


def test_widths_above_64_are_refused_by_name(lib):
    rc, msg = call(lib, widths=(65, 16))
    assert rc == GAE_E_RANGE and "layer 0" in msg and "65" in msg
    rc, msg = call(lib, widths=(32, 65))
    assert rc == GAE_E_RANGE and "layer 1" in msg and "65" in msg
    rc, msg = call(lib, f_in=65, dtype=F32, ldf=68)
    assert rc == GAE_E_RANGE and "f_in = 65" in msg
    rc, msg = call(lib, widths=(32, 0))
    assert rc == GAE_E_RANGE and "layer 1" in msg
    rc, msg = call(lib, max_nodes=65)
    assert rc == GAE_E_RANGE and "max_graph_nodes = 65" in msg


def test_short_leading_dimensions_are_refused(lib):
    rc, msg = call(lib, ldo=47)
    assert rc == GAE_E_SIZE and "ldo 47" in msg and "3 d = 48" in msg
    rc, msg = call(lib, ldw=(38, 32))
    assert rc == GAE_E_SIZE and "ldw = 38" in msg and "layer 0" in msg
    rc, msg = call(lib, ldf=39)
    assert rc == GAE_E_SIZE and "ldf = 39" in msg
    rc, msg = call(lib, dtype=F32, ldf=39)
    assert rc == GAE_E_SIZE and "ldf = 39" in msg


def test_unknown_codes_are_refused(lib):
    rc, msg = call(lib, norm=2)
    assert rc == GAE_E_RANGE and "norm code 2" in msg
    rc, msg = call(lib, norm=-1)
    assert rc == GAE_E_RANGE and "norm" in msg
    rc, msg = call(lib, acts=(1, 7))
    assert rc == GAE_E_DTYPE and "activation code 7" in msg and "layer 1" in msg
    rc, msg = call(lib, dtype=1)
    assert rc == GAE_E_DTYPE and "dtype 1" in msg


SHAPES = [  # f_in, widths, max nodes, taken?
    (39, (32, 16), 38, True), (39, (16,), 64, True), (39, (64, 32, 16), 1, True), (39, (32, 32, 32, 8), 0, True),
    (64, (64, 64, 64, 64), 64, True), (1, (1,), 1, True),
    (39, (), 38, False), (39, (32, 32, 32, 32, 16), 38, False), (39, (128, 64), 38, False), (39, (32, 65), 38, False),
    (65, (32, 16), 38, False), (0, (32, 16), 38, False), (39, (32, 0), 38, False), (39, (32, 16), 65, False),
    (39, (32, 16), 70, False),
]


@pytest.mark.parametrize("f_in,widths,max_nodes,taken", SHAPES)
def test_usable_query_agrees_with_the_refusals(lib, f_in, widths, max_nodes, taken):
    from gae_dgl_amd import ops
    assert ops.embed_graphs_usable(f_in, widths, max_nodes) is taken
    q = 16                                                            # uint8 rows: whole 16-byte vectors
    rc, msg = call(lib, widths=widths, f_in=f_in, max_nodes=max_nodes, n_layers=len(widths),
                   ldf=(max(f_in, 1) + q - 1) // q * q)
    assert (rc == GAE_OK) is taken, msg
    if not taken:
        assert rc == GAE_E_RANGE and ("outside" in msg or "above" in msg)
    assert lib.gae_embed_graphs_usable(f_in, len(widths), None, max_nodes) == 0      # no widths: never usable
    assert lib.gae_embed_graphs_usable(39, 2, (ctypes.c_int64 * 2)(32, 16), -1) == 0


def test_wrapper_refuses_cpu_tensors():
    import torch
    from gae_dgl_amd import ops
    from gae_dgl_amd._lib import GaeHipError
    gp = torch.tensor([0, 2], dtype=torch.int64)
    ip = torch.tensor([0, 1, 2], dtype=torch.int32)
    ix = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(GaeHipError, match="no CPU fallback"):
        ops.embed_graphs(gp, ip, ix, torch.zeros(2, 4), [torch.zeros(3, 4)], [None], [0])


def test_model_api_checks_its_arguments_before_touching_data():
    import gae_dgl_amd as G
    m = G.GAE(39, [32, 16])
    with pytest.raises(ValueError, match="fused"):
        m.embed_graphs(None, fused="yes")
    with pytest.raises(ValueError, match="batch_size"):
        m.embed_graphs(None, batch_size=0)


# ------------------------------------------------------------------ the command line
def _parser_error(capsys, argv):
    from gae_dgl_amd import embed as E
    with pytest.raises(SystemExit) as e:
        E.parse_args(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


BASE = ["--checkpoint", "ep09.pkl", "--hidden_dims", "32", "16", "--out", "features.npy"]


def test_cli_accepts_the_documented_command_lines():
    from gae_dgl_amd import embed as E
    a = E.parse_args(BASE + ["--synthetic", "600", "--seed", "3"])
    assert (a.checkpoint, a.hidden_dims, a.in_dim, a.synthetic, a.seed) == ("ep09.pkl", [32, 16], 39, 600, 3)
    assert (a.norm, a.fused, a.batch_size, a.gpu_id, a.data_file) == ("none", "auto", 4096, 0, None)
    a = E.parse_args(BASE + ["--data_file", "graphs.npz", "--norm", "both", "--fused", "on", "--batch_size", "128",
                             "--in_dim", "39", "--gpu_id", "1"])
    assert (a.data_file, a.norm, a.fused, a.batch_size, a.gpu_id, a.synthetic) == ("graphs.npz", "both", "on", 128, 1, 0)
    a = E.parse_args(["--checkpoint", "c.pkl", "--hidden_dims", "128", "64", "--out", "o.npy", "--synthetic", "5"])
    assert a.fused == "auto" and a.hidden_dims == [128, 64]          # wide models are fine outside --fused on


def test_cli_refuses_a_missing_checkpoint(capsys):
    err = _parser_error(capsys, ["--hidden_dims", "32", "16", "--out", "f.npy", "--synthetic", "10"])
    assert "--checkpoint" in err


def test_cli_refuses_both_and_neither_data_source(capsys):
    err = _parser_error(capsys, BASE + ["--synthetic", "10", "--data_file", "graphs.npz"])
    assert "--data_file" in err and "--synthetic" in err
    err = _parser_error(capsys, BASE)
    assert "--data_file" in err and "--synthetic" in err


def test_cli_refuses_fused_on_with_a_wide_model(capsys):
    err = _parser_error(capsys, ["--checkpoint", "c.pkl", "--hidden_dims", "128", "64", "--out", "o.npy", "--synthetic", "5",
                                 "--fused", "on"])
    assert "--fused on" in err and "128" in err


def test_cli_refuses_missing_widths_and_output(capsys):
    assert "--hidden_dims" in _parser_error(capsys, ["--checkpoint", "c.pkl", "--out", "o.npy", "--synthetic", "5"])
    assert "--out" in _parser_error(capsys, ["--checkpoint", "c.pkl", "--hidden_dims", "32", "16", "--synthetic", "5"])
