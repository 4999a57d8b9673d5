"""K33 on the device (gae_fingerprint_graphs, ops.fingerprint_graphs, DeviceGraphDataset.fingerprints) bit for bit against
the numpy restatement tests/fingerprint_ref.py.  The set is ``zinc_like(300)`` joined with the hand-made graphs of
``fingerprint_ref.joined_set``: a single atom, an empty graph, graphs of 64 .. 300 atoms (a wave's stride and its tails),
a hub of degree 100, duplicate bonds and a CSR row with a column of another graph."""
import numpy as np
import pytest
import torch

import fingerprint_ref as R

pytestmark = pytest.mark.gpu
RADII, WIDTHS = [0, 1, 2, 4, 8], [64, 1024, 2048]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


class Set:
    """the joined set on the host and the device, and the reference's atom ids (computed once, to radius 8)"""

    def __init__(self, dev):
        self.gp, self.src, self.dst, self.feat, self.first_made = R.joined_set(0)
        self.N, self.G = int(self.gp[-1]), len(self.gp) - 1
        self.ip, self.ix = R.csr_of(self.N, self.src, self.dst)
        self.d_gp = torch.from_numpy(self.gp).to(dev)
        self.d_ip, self.d_ix = torch.from_numpy(self.ip).to(dev), torch.from_numpy(self.ix).to(dev)
        self.d_f32 = torch.from_numpy(self.feat).to(dev)
        self.d_u8 = torch.from_numpy(self.feat.astype(np.uint8)).to(dev)
        self.ids = R.atom_ids(self.gp, self.ip, self.ix, self.feat, 8)

    def counts(self, radius, n_bits, graph_ids=None):
        gids = np.arange(self.G) if graph_ids is None else np.asarray(graph_ids)
        out = np.zeros((len(gids), n_bits), dtype=np.int32)
        for k, g in enumerate(gids):
            if 0 <= g < self.G:
                slots = (self.ids[:radius + 1, self.gp[g]:self.gp[g + 1]] & np.uint64(n_bits - 1)).astype(np.int64)
                np.add.at(out[k], slots.reshape(-1), 1)
        return out


@pytest.fixture(scope="module")
def mols(dev):
    return Set(dev)


def as_np(t):
    return t.detach().cpu().numpy()


def test_the_set_holds_what_it_should(mols):
    sizes = np.diff(mols.gp)[mols.first_made:].tolist()
    assert sizes == [1, 5, 0, 7, 64, 65, 70, 257, 300, 101, 6, 8]
    deg = np.diff(mols.ip)
    assert deg.max() == 100
    lo = np.repeat(mols.gp[:-1], np.diff(mols.gp))[np.repeat(np.arange(mols.N), deg)]
    assert ((mols.ix < lo)).sum() == 1                                 # the one column of another graph
    assert np.array_equal(mols.counts(2, 128), R.fingerprint_counts(mols.gp, mols.ip, mols.ix, mols.feat, 2, 128))


@pytest.mark.parametrize("n_bits", WIDTHS)
@pytest.mark.parametrize("radius", RADII)
def test_bits_and_counts_in_both_storages(mols, radius, n_bits):
    from gae_dgl_amd import ops
    want = mols.counts(radius, n_bits)
    for feat in (mols.d_u8, mols.d_f32):
        c = ops.fingerprint_graphs(mols.d_gp, mols.d_ip, mols.d_ix, feat, radius=radius, n_bits=n_bits, counts=True)
        b = ops.fingerprint_graphs(mols.d_gp, mols.d_ip, mols.d_ix, feat, radius=radius, n_bits=n_bits)
        assert c.dtype == torch.int32 and c.shape == (mols.G, n_bits) and b.shape == (mols.G, n_bits // 32)
        assert np.array_equal(as_np(c), want), np.argwhere(as_np(c) != want)[:4]
        assert np.array_equal(as_np(b), R.pack_bits(want > 0))
    empty = mols.first_made + 2
    assert not want[empty].any() and want[mols.first_made].sum() == radius + 1


def test_non_binary_features_with_negative_zero_and_non_finite_values(mols, dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((mols.N, 7)).astype(np.float32)
    feat[rng.random(feat.shape) < 0.2] = -0.0
    feat[3, 1], feat[40, 0], feat[41, 6] = np.nan, np.inf, -np.inf
    assert np.signbit(feat[feat == 0]).any()
    got = ops.fingerprint_graphs(mols.d_gp, mols.d_ip, mols.d_ix, torch.from_numpy(feat).to(dev), radius=2, n_bits=1024,
                                 counts=True)
    assert np.array_equal(as_np(got), R.fingerprint_counts(mols.gp, mols.ip, mols.ix, feat, 2, 1024))
    pos = np.where(feat == 0, np.float32(0), feat)
    again = ops.fingerprint_graphs(mols.d_gp, mols.d_ip, mols.d_ix, torch.from_numpy(pos).to(dev), radius=2, n_bits=1024,
                                   counts=True)
    assert torch.equal(got, again)


def test_graph_ids_permuted_repeated_and_out_of_range(mols, dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(1)
    gids = np.concatenate([rng.permutation(mols.G), rng.integers(0, mols.G, 50), [mols.G - 4, mols.G - 4, -1, mols.G, 0]])
    got = ops.fingerprint_graphs(mols.d_gp, mols.d_ip, mols.d_ix, mols.d_u8, radius=2, n_bits=1024, counts=True,
                                 graph_ids=torch.from_numpy(gids).to(dev))
    want = mols.counts(2, 1024, gids)
    assert np.array_equal(as_np(got), want)
    assert not want[-3].any() and not want[-2].any() and want[-1].any()


def test_bad_node_ranges_and_row_pointers_give_zero_rows_and_empty_rows(mols, dev):
    from gae_dgl_amd import ops
    gp = mols.gp.copy()
    gp[-1] = mols.N + 3                                                # the last graph's range leaves the set
    got = ops.fingerprint_graphs(torch.from_numpy(gp).to(dev), mols.d_ip, mols.d_ix, mols.d_u8, radius=2, n_bits=64,
                                 counts=True)
    want = mols.counts(2, 64)
    want[-1] = 0
    assert np.array_equal(as_np(got), want)
    # a row pointer beyond E: row v ends there and row v + 1 starts there -- both read as empty rows
    v = int(mols.gp[mols.first_made + 4]) + 10
    ip = mols.ip.copy()
    ip[v + 1] = len(mols.ix) + 5
    got = ops.fingerprint_graphs(mols.d_gp, torch.from_numpy(ip).to(dev), mols.d_ix, mols.d_u8, radius=2, n_bits=64,
                                 counts=True)
    keep = (mols.dst != v) & (mols.dst != v + 1)
    ip2, ix2 = R.csr_of(mols.N, mols.src[keep], mols.dst[keep])
    assert np.array_equal(as_np(got), R.fingerprint_counts(mols.gp, ip2, ix2, mols.feat, 2, 64))


def test_strided_features_whose_pad_holds_nan_and_two_runs(mols, dev):
    from gae_dgl_amd import ops
    buf = torch.full((mols.N, 39 + 5), float("nan"), dtype=torch.float32)
    buf[:, :39] = torch.from_numpy(mols.feat)
    view = buf.to(dev)[:, :39]
    assert view.stride(0) == 44
    a = ops.fingerprint_graphs(mols.d_gp, mols.d_ip, mols.d_ix, view, radius=4, n_bits=1024)
    b = ops.fingerprint_graphs(mols.d_gp, mols.d_ip, mols.d_ix, view, radius=4, n_bits=1024)
    assert torch.equal(a, b) and np.array_equal(as_np(a), R.pack_bits(mols.counts(4, 1024) > 0))
    pad8 = torch.full((mols.N, 48), 255, dtype=torch.uint8)
    pad8[:, :39] = torch.from_numpy(mols.feat.astype(np.uint8))
    assert torch.equal(ops.fingerprint_graphs(mols.d_gp, mols.d_ip, mols.d_ix, pad8.to(dev)[:, :39], radius=4, n_bits=1024), a)


@pytest.mark.parametrize("counts", [False, True])
def test_canary_rows_and_columns_stay_untouched(mols, dev, counts):
    from gae_dgl_amd import _lib
    from gae_dgl_amd.ops import _ptr, _stream
    n_bits, B = 128, mols.G
    width = n_bits if counts else n_bits // 32
    out = torch.full((B + 2, width + 3), -7, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.load().gae_fingerprint_workspace_bytes(mols.N), dtype=torch.uint8, device=dev)
    _lib.call("gae_fingerprint_graphs", _ptr(mols.d_gp), mols.G, mols.N, len(mols.ix), _ptr(mols.d_ip), _ptr(mols.d_ix),
              _ptr(mols.d_u8), _lib.U8, 39, 39, None, B, 2, n_bits, int(counts), _ptr(out[1:]), width + 3, _ptr(ws),
              ws.numel(), _stream())
    torch.cuda.synchronize()
    assert bool((out[0] == -7).all()) and bool((out[-1] == -7).all()) and bool((out[:, width:] == -7).all())
    want = mols.counts(2, n_bits)
    assert np.array_equal(as_np(out[1:-1, :width]), want if counts else R.pack_bits(want > 0))


def test_dataset_subset_views_and_batched_graphs(dev):
    from gae_dgl_amd import ops, workloads
    from gae_dgl_amd.dataset import DeviceGraphDataset
    gp, src, dst, X = workloads.zinc_like(300, 2)
    ip, ix = R.csr_of(int(gp[-1]), src, dst)
    want = R.fingerprint_counts(gp, ip, ix, X, 2, 1024)
    for storage in ("uint8", "float32"):
        data = DeviceGraphDataset(gp, src, dst, X, device=dev, feat_storage=storage)
        assert np.array_equal(as_np(data.fingerprints(counts=True)), want)
        assert np.array_equal(as_np(data.fingerprints()), R.pack_bits(want > 0))
        ids = np.array([5, 299, 0, 5, 17], dtype=np.int64)
        sub = data.subset(ids)
        assert np.array_equal(as_np(sub.fingerprints(radius=1, n_bits=64, counts=True)),
                              R.fingerprint_counts(gp, ip, ix, X, 1, 64, ids))
    g = data.batch([7, 3, 250])
    got = DeviceGraphDataset.fingerprints(g, radius=2, n_bits=1024, counts=True)
    assert np.array_equal(as_np(got), want[[7, 3, 250]])
    folded = ops.fingerprint_fold(data.fingerprints(counts=True), 128)
    assert torch.equal(folded, data.fingerprints(n_bits=128, counts=True))
    assert torch.equal(ops.fingerprint_unpack(data.fingerprints(n_bits=128)), (folded > 0).float())
