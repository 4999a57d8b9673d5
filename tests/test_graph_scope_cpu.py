"""CPU-side checks of the per-member reconstruction loss (scope="graph", gae_decoder_bce_graphs): the reference-generated
fixture against an fp64 restatement, the entry points' argument errors (no GPU needed), the C ABI and the refusals of
the Python and command-line interfaces."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------- the fixture, restated in fp64
def _molecule_loss64(W, b, n, src, dst, X, mask):
    """train_inductive.py:44-48 on ONE molecule, fp64: GCN layers (in-edge sum, Linear, ReLU but on the last), the
    inner-product decoder on Z (.) mask, the molecule's own label and pos_weight"""
    h = torch.from_numpy(X).double()
    s, d = torch.from_numpy(src), torch.from_numpy(dst)
    for li, (w, bb) in enumerate(zip(W, b)):
        h = torch.zeros(n, h.shape[1], dtype=torch.float64).index_add(0, d, h[s])
        h = h @ w.T + bb
        if li < len(W) - 1:
            h = torch.relu(h)
    z = h if mask is None else h * torch.from_numpy(mask).double()
    x = z @ z.T
    y = torch.zeros(n, n, dtype=torch.float64).index_put((d, s), torch.ones(len(src), dtype=torch.float64),
                                                          accumulate=True)
    pw = (n * n - y.sum()) / y.sum()
    return ((1 - y) * x + (1 + (pw - 1) * y) * torch.nn.functional.softplus(-x)).mean()


def test_fixture_matches_fp64_restatement():
    fx, whole, parts = load_golden("mol8_graph_scope"), load_golden("mol8"), load_golden("mol8_parts")
    L = len(whole["hidden"])
    names = [f"layers.{i}.apply_mod.linear.{w}" for i in range(L) for w in ("weight", "bias")]
    offs = fx["node_ptr"]
    assert offs[-1] == int(whole["n"]) and len(offs) == int(parts["n_graphs"]) + 1
    for tag, use_mask in (("p0", False), ("p01", True)):
        params = {k: torch.from_numpy(whole["sd/" + k]).double().requires_grad_() for k in names}
        W = [params[f"layers.{i}.apply_mod.linear.weight"] for i in range(L)]
        b = [params[f"layers.{i}.apply_mod.linear.bias"] for i in range(L)]
        per = []
        for i in range(len(offs) - 1):
            m = whole["mask"][offs[i]:offs[i + 1]] if use_mask else None
            per.append(_molecule_loss64(W, b, int(parts[f"g{i}/n"]), parts[f"g{i}/src"], parts[f"g{i}/dst"],
                                        parts[f"g{i}/X"], m))
        loss = torch.stack(per).mean()
        loss.backward()
        assert abs(float(loss.detach()) - float(fx["loss_" + tag])) < 1e-5 * max(1.0, abs(float(loss.detach())))
        assert np.allclose(torch.stack(per).detach().numpy(), fx["graph_loss_" + tag], rtol=1e-5, atol=1e-6)
        for k in names:
            ref = params[k].grad.numpy()
            err = np.abs(fx[f"grad_{tag}/{k}"] - ref).max() / max(np.abs(ref).max(), 1.0)
            assert err < 1e-5, (tag, k, err)
    # the per-member loss is a different quantity from the batch loss of the same graph
    assert abs(float(fx["loss_p0"]) - float(whole["loss_p0"])) > 1e-3


# ----------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib.load()


def test_entry_points_declared_and_bound(lib):
    from gae_dgl_amd import _lib
    text = open(os.path.join(ROOT, "include", "gae_hip.h")).read()
    for name in ("gae_decoder_bce_graphs_workspace_bytes", "gae_decoder_bce_graphs"):
        assert f"{name}(" in text and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "train_inductive.py:44-48" in text[text.index("K15: the same loss"):text.index("gae_decoder_bce_graphs(")]


def _call(lib, **kw):
    """gae_decoder_bce_graphs with a valid-looking argument set (fake, never dereferenced device pointers) and the
    overrides in ``kw``; every case below must be refused before any launch"""
    fake = ctypes.c_void_p(1 << 40)
    a = dict(Z=fake, mask=None, ldz=16, n=100, d=16, node_ptr=fake, G=4, M=40, indptr=fake, indices=fake,
             t_indptr=fake, t_indices=fake, counts=None, p=0.0, seed=0, offset=0, draw=None, loss=fake, gl=None,
             dZ=fake, lddz=16, ws=fake, ws_bytes=1 << 20, sync=fake)
    a.update(kw)
    return lib.gae_decoder_bce_graphs(a["Z"], a["mask"], a["ldz"], a["n"], a["d"], a["node_ptr"], a["G"], a["M"],
                                      a["indptr"], a["indices"], a["t_indptr"], a["t_indices"], a["counts"], a["p"],
                                      a["seed"], a["offset"], a["draw"], a["loss"], a["gl"], a["dZ"], a["lddz"],
                                      a["ws"], a["ws_bytes"], a["sync"], None)


def test_argument_errors_without_gpu(lib):
    GAE_E_NULL, GAE_E_SIZE, GAE_E_WORKSPACE, GAE_E_RANGE = -1, -2, -5, -6
    assert lib.gae_decoder_bce_graphs_workspace_bytes(-1, 4, 40, 16) == GAE_E_SIZE
    assert lib.gae_decoder_bce_graphs_workspace_bytes(100, -4, 40, 16) == GAE_E_SIZE
    assert lib.gae_decoder_bce_graphs_workspace_bytes(100, 4, 40, 65) == GAE_E_RANGE
    small = lib.gae_decoder_bce_graphs_workspace_bytes(100, 4, 40, 16)
    big = lib.gae_decoder_bce_graphs_workspace_bytes(100, 4, 300, 16)
    assert 0 < small < big                                    # members above 64 rows add panel items
    assert _call(lib, n=-1) == GAE_E_SIZE
    assert _call(lib, d=-1) == GAE_E_SIZE
    assert _call(lib, G=-1) == GAE_E_SIZE
    assert _call(lib, M=-1) == GAE_E_SIZE
    assert _call(lib, d=65, ldz=65, lddz=65) == GAE_E_RANGE
    assert _call(lib, ldz=8) == GAE_E_SIZE
    assert _call(lib, node_ptr=None) == GAE_E_NULL
    assert _call(lib, sync=None) == GAE_E_NULL
    assert _call(lib, t_indptr=None) == GAE_E_NULL
    assert _call(lib, p=0.5) == GAE_E_NULL                    # in-launch dropout needs the mask output
    assert _call(lib, p=1.0, mask=ctypes.c_void_p(1 << 40)) == GAE_E_RANGE
    assert _call(lib, ws_bytes=small - 1) == GAE_E_WORKSPACE
    assert _call(lib, ws_bytes=big - 1, M=300) == GAE_E_WORKSPACE
    assert b"gae_decoder_bce_graphs" in lib.gae_last_error()


# ----------------------------------------------------------------- Python / CLI refusals
def test_scope_refusals():
    import gae_dgl_amd as G
    model = G.GAE(5, [4, 3])
    with pytest.raises(ValueError, match="scope"):
        model.reconstruction_loss(object(), scope="molecule")
    with pytest.raises(ValueError, match="criterion"):
        model.reconstruction_loss(object(), criterion="mse", scope="graph")
    from gae_dgl_amd.capture import CapturedInductiveStep
    with pytest.raises(ValueError, match="loss_scope"):
        CapturedInductiveStep(model, None, None, 1, loss_scope="pairs")


@pytest.mark.parametrize("extra", [["--criterion", "mse"], ["--loss", "dense"]])
def test_cli_refuses_graph_scope_combinations(extra, capsys):
    from gae_dgl_amd import train_inductive
    with pytest.raises(SystemExit) as e:
        train_inductive.main(["--loss_scope", "graph", "--synthetic", "10", "--no_plot"] + extra)
    assert e.value.code == 2
    assert "--loss_scope graph" in capsys.readouterr().err


def test_cli_scope_flag():
    from gae_dgl_amd import train_inductive
    ap = train_inductive.build_parser()
    assert ap.parse_args([]).loss_scope == "batch"
    assert ap.parse_args(["--loss_scope", "graph"]).loss_scope == "graph"
    with pytest.raises(SystemExit):
        ap.parse_args(["--loss_scope", "pairs"])
