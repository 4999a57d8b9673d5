"""The balanced schedule of the symmetric fused loss (256-row panels, the Pubmed default) walks the edges in blocks
appended to its dense launch; the edge kernel behind it only folds the mirror strips and assembles dZ.  Loss and
gradient against the fp64 oracle, bits stable from call to call, and the fp16 range guard's fallback launch still
giving the three-piece bf16 results."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5


def _graph(n, seed=0, deg=4, hubs=3, hub_deg=150):
    """random symmetric edges plus a few hub rows longer than the walk's per-group limit (16 edges)"""
    import gae_dgl_amd as G
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, deg * n); dst = rng.integers(0, n, deg * n)
    hs = np.repeat(rng.integers(0, n, hubs), hub_deg); hd = rng.integers(0, n, hubs * hub_deg)
    src = np.concatenate([src, hs]); dst = np.concatenate([dst, hd])
    g = G.DGLGraph((np.concatenate([src, dst]), np.concatenate([dst, src])), num_nodes=n).to(DEV)
    return g


def _oracle(Zt, g, pw, window=2048):
    from oracle import gae_oracle as O
    ip, ix = (t.cpu().numpy() for t in g.csr())
    tp, tx = (t.cpu().numpy() for t in g.csc())
    n = Zt.shape[0]
    loss, grads = 0.0, []
    for r0 in range(0, n, window):
        l, gr = O.bce_row_window(Zt, r0, min(n, r0 + window), ip, ix, tp, tx, pw)
        loss += float(l); grads.append(gr)
    return loss, torch.cat(grads)


def _rel(a, b):
    a = torch.as_tensor(a).double().cpu(); b = torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _call(Z, g, pw, dropout):
    from gae_dgl_amd import ops
    mask = torch.empty_like(Z) if dropout else None
    draws = torch.zeros(1, dtype=torch.int64, device=DEV)
    drop = (0.1, 7, 0, draws) if dropout else None
    loss, dz = ops.decoder_bce_raw(Z, mask, g.csr(), g.csc(), pw, True, dropout=drop)
    torch.cuda.synchronize()
    return loss, dz, mask


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("n", [8000, 19717])
def test_balanced_loss_with_walk_blocks_matches_oracle(n, dropout):
    from gae_dgl_amd import _lib
    g = _graph(n, seed=n)
    E = g.number_of_edges()
    pw = (n * n - E) / E
    torch.manual_seed(3)
    Z = torch.randn(n, 16, device=DEV) * 0.3
    loss, dz, mask = _call(Z, g, pw, dropout)
    assert _lib.tuning_get("bce_last_kind") == 3, "the loss did not run on the balanced symmetric kernel"
    loss2, dz2, mask2 = _call(Z, g, pw, dropout)
    assert torch.equal(loss, loss2) and torch.equal(dz, dz2), "two calls differ"
    m = mask.double().cpu() if dropout else torch.ones(n, 16, dtype=torch.float64)
    Zt = Z.double().cpu() * m
    ref_loss, ref_dzt = _oracle(Zt, g, pw)
    assert abs(float(loss) - ref_loss) <= TOL * max(1.0, abs(ref_loss)), (float(loss), ref_loss)
    assert _rel(dz, ref_dzt * m) < TOL


def test_range_guard_fallback_equals_three_piece_bf16(tuning):
    """|Zt| > 65504 fires the fp16 guard: the fallback launch recomputes the dense part in three bf16 pieces and must
    give exactly what the three-piece launch (knob bce_s_bf16 = 2) gives; the walk blocks' results stand either way"""
    n = 8000
    g = _graph(n, seed=11)
    E = g.number_of_edges()
    pw = (n * n - E) / E
    torch.manual_seed(4)
    Z = torch.randn(n, 16, device=DEV) * 0.3
    Z[123, 5] = 7.0e4
    loss_g, dz_g, _ = _call(Z, g, pw, False)          # default: fp16 pieces, guard fires, fallback recomputes
    tuning("bce_s_bf16", 2)
    loss_b, dz_b, _ = _call(Z, g, pw, False)
    assert torch.isfinite(loss_b).all() and torch.isfinite(dz_b).all()
    assert torch.equal(loss_g, loss_b) and torch.equal(dz_g, dz_b)
