"""K18 on the MI355X: gae_decoder_rank / ops.decoder_rank / GAE.rank_links against the dense fp64 reference of
tests/rank_ref.py -- bit for bit where fp32 is exact, inside an fp64 sandwich on random fp32 embeddings -- and against
gae_decoder_topk, whose scores it must reproduce bit for bit."""
import numpy as np
import pytest
import torch

from conftest import CASES, load_golden
from rank_ref import rank_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need an MI355X"
    return torch.device("cuda:0")


def as_np(t):
    return t.detach().cpu().numpy()


def host_csr(g):
    indptr, indices = g.csr()
    return as_np(indptr).astype(np.int64), as_np(indices).astype(np.int64)


def dev_csr(csr, dev):
    return (torch.as_tensor(csr[0], dtype=torch.int32, device=dev), torch.as_tensor(csr[1], dtype=torch.int32, device=dev))


def same_scores(a, b):
    """fp32 arrays equal bit for bit up to the sign of zero, NaN where NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def assert_equal_ref(res, ref, what=""):
    score, greater, equal, cand = ref
    assert same_scores(as_np(res.score), score.astype(np.float32)), what
    assert np.array_equal(as_np(res.greater), greater), what
    assert np.array_equal(as_np(res.equal), equal), what
    assert np.array_equal(as_np(res.candidates), cand), what


def _random_csr(rng, n, deg_max, hubs=(), full_rows=(), sort_rows=False):
    rows = []
    for i in range(n):
        if i in full_rows:
            r = np.arange(n)
        elif i in hubs:
            r = rng.choice(n, size=min(170, n), replace=False)
        else:
            r = rng.integers(0, n, rng.integers(0, deg_max + 1))
        if r.size > 1:
            r = np.concatenate([r, r[:2]])               # repeated entries
        rng.shuffle(r)                                    # any order
        if sort_rows:
            r = np.sort(r)                                # the kernel's O(1) first-occurrence test
        rows.append(r)
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([r.size for r in rows])
    indices = np.concatenate(rows) if n else np.zeros(0, np.int64)
    return indptr, indices.astype(np.int64)


def _windows(n):
    """three members, the middle one empty: (node_ptr, windows [n, 2])"""
    gp = np.array([0, n // 3, n // 3, n], dtype=np.int64)
    member = np.searchsorted(gp, np.arange(n), side="right") - 1
    return gp, np.stack([gp[member], gp[member + 1]], 1)


def _queries(rng, n, m, csr, windows):
    """m random queries (sources repeat) with, where m allows, targets that are the source itself, known edges of the
    source and nodes outside the source's window"""
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    if m >= 16:
        src[1] = src[0]                                   # a shared source
        dst[2] = src[2]                                   # self
        dst[3] = src[3]
        k = 4
        if csr is not None:
            deg = np.diff(csr[0])
            for i in np.flatnonzero(deg > 0)[:3]:         # a known edge as the target
                src[k], dst[k] = i, csr[1][csr[0][i]]
                k += 1
        if windows is not None and n >= 3:
            src[k], dst[k] = 0, n - 1                     # the target lies in another member
            src[k + 1], dst[k + 1] = n - 1, 0
    return src.astype(np.int64), dst.astype(np.int64)


def _exact_case(n, d, ms, dev, seed, ld_pad=3, exclude_self=True, with_edges=True, graph_scope=False, hubs=(),
                full_rows=(), sort_rows=False):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(seed)
    Zi = rng.integers(-2, 3, (n, d)).astype(np.float32)
    if n > 4:
        Zi[n // 2] = Zi[1]                                # equal rows: ties everywhere
    buf = torch.zeros(n, d + ld_pad, dtype=torch.float32, device=dev)
    buf[:, :d] = torch.from_numpy(Zi)
    Z = buf[:, :d]                                        # strided: ldz > d
    csr = _random_csr(rng, n, 6, hubs, full_rows, sort_rows) if with_edges else None
    dcsr = dev_csr(csr, dev) if csr is not None else None
    gp, windows = _windows(n) if graph_scope else (None, None)
    node_ptr = torch.as_tensor(gp, device=dev) if gp is not None else None
    bound = int(np.diff(gp).max()) if gp is not None else 0
    for m in ms:
        src, dst = _queries(rng, n, m, csr, windows)
        res = ops.decoder_rank_raw(Z, torch.as_tensor(src, device=dev), torch.as_tensor(dst, device=dev), node_ptr,
                                   bound, dcsr, exclude_self=exclude_self)
        assert res.score.shape == (m,) and res.greater.dtype == torch.int64
        assert_equal_ref(res, rank_ref(Zi, src, dst, windows, csr, exclude_self), (n, d, m, graph_scope))


# ------------------------------------------------------------------ exact integer cases: bit for bit
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130, 2708])
@pytest.mark.parametrize("d", [1, 3, 16, 17, 64, 256])
def test_exact_integer_case_bit_for_bit(n, d, dev):
    hubs = (3,) if n > 3 else ()
    full = (5,) if n > 5 else ()
    ms = (0, 1, 31, 32, 33, 1000)
    _exact_case(n, d, ms, dev, seed=n * 1000 + d, hubs=hubs, full_rows=full)
    _exact_case(n, d, (33, 200), dev, seed=n * 1000 + d + 1, hubs=hubs, full_rows=full, sort_rows=True)
    _exact_case(n, d, (1, 64, 300), dev, seed=n * 1000 + d + 2, graph_scope=True, hubs=hubs, full_rows=full)


def test_hub_and_full_row_sources(dev):
    """every query's source is a hub row or the row whose CSR lists every node (shuffled, with repeats: the scan for
    the first occurrence), targets inside and outside the row"""
    from gae_dgl_amd import ops
    rng = np.random.default_rng(7)
    n, d = 300, 16
    Zi = rng.integers(-2, 3, (n, d)).astype(np.float32)
    Zi[200] = Zi[10]
    for sort_rows in (False, True):
        csr = _random_csr(rng, n, 6, hubs=(3, 77, 150), full_rows=(5, 299), sort_rows=sort_rows)
        src = rng.choice([3, 77, 150, 5, 299], 200).astype(np.int64)
        dst = rng.integers(0, n, 200).astype(np.int64)
        for ex in (True, False):
            res = ops.decoder_rank_raw(torch.from_numpy(Zi).to(dev), torch.as_tensor(src, device=dev),
                                       torch.as_tensor(dst, device=dev), None, 0, dev_csr(csr, dev), exclude_self=ex)
            ref = rank_ref(Zi, src, dst, None, csr, ex)
            assert_equal_ref(res, ref, (sort_rows, ex))
            full = np.isin(src, [5, 299])
            assert (ref[3][full] == 0).all()              # the whole window is filtered: no candidate, rank 1


def test_flags_alone_and_together(dev):
    for ex in (True, False):
        for edges in (True, False):
            _exact_case(300, 16, (100,), dev, seed=11 + 2 * ex + edges, exclude_self=ex, with_edges=edges, hubs=(4,),
                        full_rows=(9,))
            _exact_case(300, 5, (100,), dev, seed=21 + 2 * ex + edges, exclude_self=ex, with_edges=edges,
                        graph_scope=True)


def build_model(g, dev):
    import gae_dgl_amd as G
    model = G.GAE(g["X"].shape[1], [int(h) for h in g["hidden"]])
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd/")})
    return model.to(dev)


def fresh_graph(g, dev):
    import gae_dgl_amd as G
    gr = G.DGLGraph()
    gr.add_nodes(int(g["n"]))
    gr.add_edges(g["src"], g["dst"])
    gr.to(dev)
    gr.ndata['h'] = torch.from_numpy(g["X"]).to(dev)
    return gr


def test_single_member_graph_scope_equals_batch_scope(dev):
    g = load_golden("sym200")
    model = build_model(g, dev)
    n = int(g["n"])
    pairs = np.random.default_rng(0).integers(0, n, (2, 500))
    a = model.rank_links(fresh_graph(g, dev), pairs, scope="graph")
    b = model.rank_links(fresh_graph(g, dev), pairs)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ------------------------------------------------------------------ the same number K16 computes
def test_scores_and_ranks_agree_with_topk(dev):
    """for every entry (i, r) of gae_decoder_topk's lists the query (i, index[i, r]) returns the list's score bit for
    bit and a rank interval that holds r"""
    from gae_dgl_amd import ops
    torch.manual_seed(5)
    rng = np.random.default_rng(5)
    n, d, k = 19717, 16, 64
    Z = torch.randn(n, d, device=dev)
    deg = 5
    indptr = np.arange(n + 1, dtype=np.int64) * deg
    indices = rng.integers(0, n, n * deg).astype(np.int64)
    dcsr = dev_csr((indptr, indices), dev)
    score, index = ops.decoder_topk_raw(Z, k, None, 0, dcsr, exclude_self=True)
    rows = torch.arange(n, device=dev).unsqueeze(1).expand_as(index)
    ok = index >= 0
    src, dst, pos = rows[ok].contiguous(), index[ok].contiguous(), torch.arange(k, device=dev).expand_as(index)[ok]
    res = ops.decoder_rank_raw(Z, src, dst, None, 0, dcsr, exclude_self=True)
    assert src.numel() == n * k
    assert torch.equal(res.score.view(torch.int32), score[ok].view(torch.int32))
    assert bool((res.greater <= pos).all()) and bool((pos <= res.greater + res.equal).all())
    assert bool((res.candidates >= n - 2 - deg).all())


def _fma32(a, b, c):
    """fp32 fma(a, b, c) exactly: the product of two fp32 is exact in fp64, and the fp64 sum is rounded to odd (TwoSum
    tells whether it was exact), so that the rounding to fp32 afterwards is the only one that counts"""
    p, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _chain_scores(Z):
    """Z Z^T as csrc/decoder_pairs.h defines it: per pair ONE fp32 fma chain from 0 over the features in the order the
    two lane halves feed them -- of every 2 DH-wide chunk feature s of the lower half, then of the upper, s ascending;
    DH = 8, 16, 32 for d <= 16, 32, above.  fp32 [n, n], the bits both kernels must return"""
    n, d = Z.shape
    DH = 8 if d <= 16 else 16 if d <= 32 else 32
    S = np.zeros((n, n), dtype=np.float32)
    for c0 in range(0, d, 2 * DH):
        for s in range(DH):
            for f in (c0 + s, c0 + DH + s):
                if f < d:                                 # a feature past d is a zero operand: the sum stays
                    S = _fma32(Z[:, f:f + 1], Z[None, :, f], S)
    return S


@pytest.mark.parametrize("d", [3, 16, 17, 33, 64, 65, 130, 256])
def test_topk_and_rank_share_scores_small(d, dev, tuning):
    """the seam of csrc/decoder_pairs.h in every dispatch form (all four <DH, ONE> forms, with and without a feature
    tail), on ragged members whose windows start and end off the tile boundaries, in both scopes and with 1 and 3
    column splits of either kernel: the rank query of every top-k entry returns the list's score bit for bit and a
    rank interval that holds its position, and both kernels equal their CPU references (oracle_topk, rank_ref) read
    off the fp32 chain of _chain_scores: exact indices, counts and score bits"""
    from gae_dgl_amd import ops
    from test_gpu_decoder_topk import allowed_mask, oracle_topk
    sizes = [1, 2, 31, 32, 33, 70, 5]
    gp = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, k = int(gp[-1]), 8
    member = np.searchsorted(gp, np.arange(n), side="right") - 1
    windows = np.stack([gp[member], gp[member + 1]], 1)
    rng = np.random.default_rng(d)
    torch.manual_seed(d)
    Zc = torch.randn(n, d)
    Zc[120], Zc[160] = Zc[101], Zc[140]                   # bitwise copies inside the 70-node member [99, 169): ties
    rows = []
    for i in range(n):                                    # block diagonal, about three in-edges, unsorted, empty rows
        r = rng.integers(windows[i, 0], windows[i, 1], rng.integers(0, 7))
        if r.size > 1 and rng.random() < 0.3:
            r[-1] = r[0]                                  # a repeated entry
        rows.append(r)
    assert any(r.size == 0 for r in rows) and any(r.size > np.unique(r).size for r in rows)
    csr = (np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64),
           np.concatenate(rows).astype(np.int64))
    Z, dcsr, node_ptr = Zc.to(dev), dev_csr(csr, dev), torch.as_tensor(gp, device=dev)
    S = _chain_scores(Zc.numpy()).astype(np.float64)
    extra = rng.integers(0, n, (2, 64))                   # random queries: targets outside the window, self pairs
    for scope, wins in ((node_ptr, windows), (None, None)):
        sc, idx = oracle_topk(S, allowed_mask(n, wins, csr), k)
        ok = idx >= 0
        src = np.concatenate([np.nonzero(ok)[0], extra[0]])
        dst = np.concatenate([idx[ok], extra[1]])
        pos = torch.as_tensor(np.nonzero(ok)[1], device=dev)
        ref = rank_ref(Zc.numpy(), src, dst, wins, csr, True, scores=S)
        src_t, dst_t = torch.as_tensor(src, device=dev), torch.as_tensor(dst, device=dev)
        for ts in (1, 3):
            tuning("topk_splits", ts)
            score, index = ops.decoder_topk_raw(Z, k, scope, max(sizes), dcsr)
            assert np.array_equal(as_np(index), idx), (scope is None, ts)
            assert np.array_equal(as_np(score), sc.astype(np.float32)), (scope is None, ts)
            for rs in (1, 3):
                tuning("rank_splits", rs)
                res = ops.decoder_rank_raw(Z, src_t, dst_t, scope, max(sizes), dcsr)
                m = int(ok.sum())
                listed = score[torch.as_tensor(ok, device=dev)]
                assert torch.equal(res.score[:m].view(torch.int32), listed.view(torch.int32))
                assert bool((res.greater[:m] <= pos).all()) and bool((pos <= res.greater[:m] + res.equal[:m]).all())
                assert_equal_ref(res, ref, (scope is None, ts, rs))


def test_bitwise_copies_tie(dev):
    from gae_dgl_amd import ops
    torch.manual_seed(6)
    rng = np.random.default_rng(6)
    n, d = 5000, 16
    Z = torch.randn(n, d, device=dev)
    perm = rng.permutation(n)
    a, b = perm[:100], perm[100:200]
    Z[torch.as_tensor(b, device=dev)] = Z[torch.as_tensor(a, device=dev)]
    i = rng.integers(0, n, 100)
    keep = (i != a) & (i != b)                            # self is excluded: b must be a candidate of i
    res = ops.decoder_rank(Z, np.stack([i, a]))
    res_b = ops.decoder_rank(Z, np.stack([i, b]))
    keep = torch.as_tensor(keep, device=dev)
    assert bool(keep.any()) and bool((res.equal[keep] >= 1).all())
    assert torch.equal(res.score.view(torch.int32), res_b.score.view(torch.int32))
    assert torch.equal(res.greater[keep], res_b.greater[keep]) and torch.equal(res.equal[keep], res_b.equal[keep])


# ------------------------------------------------------------------ fp64 sandwich on random fp32 embeddings
def _sandwich(Z64, src, dst, chunk=64, rel=1e-6, ok_rows=None):
    """(S_ij, bound_ij, L, H) over C(i) \\ {j} with every node a candidate (or ok_rows(i0, i1) -> bool [rows, n]):
    margin_c = rel (|z_i| |z_c| + |z_i| |z_j|), L = #{S_ic - S_ij > margin_c}, H = #{S_ic - S_ij >= -margin_c}"""
    norms = Z64.norm(dim=1)
    m = len(src)
    t_all = torch.empty(m, dtype=torch.float64); tb = torch.empty(m, dtype=torch.float64)
    L = torch.empty(m, dtype=torch.int64); H = torch.empty(m, dtype=torch.int64)
    src_t, dst_t = torch.as_tensor(src), torch.as_tensor(dst)
    for q0 in range(0, m, chunk):
        i, j = src_t[q0:q0 + chunk], dst_t[q0:q0 + chunk]
        S = Z64[i] @ Z64.T
        r = torch.arange(len(i))
        t = S[r, j]
        margin = rel * (norms[i, None] * norms[None, :] + (norms[i] * norms[j])[:, None])
        diff = S - t[:, None]
        ok = torch.ones_like(S, dtype=torch.bool) if ok_rows is None else ok_rows(src[q0:q0 + chunk])
        ok[r, j] = False
        L[q0:q0 + chunk] = ((diff > margin) & ok).sum(1)
        H[q0:q0 + chunk] = ((diff >= -margin) & ok).sum(1)
        t_all[q0:q0 + chunk] = t
        tb[q0:q0 + chunk] = rel * norms[i] * norms[j]
    return t_all, tb, L, H


@pytest.mark.parametrize("n,m,seed,band", [(19717, 2048, 0, 0.25), (200_000, 512, 1, 2.0)])
def test_fp64_sandwich(n, m, seed, band, dev):
    from gae_dgl_amd import ops
    torch.manual_seed(seed)
    Zc = torch.randn(n, 16)                               # drawn on the CPU: the inputs checked below
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, m)
    dst = rng.integers(0, n, m)
    t, tb, L, H = _sandwich(Zc.double(), src, dst)
    width = (H - L).double()
    print(f"n = {n}: band mean {float(width.mean()):.3f} max {int(width.max())}, ranks up to {int(H.max())}")
    assert float(width.mean()) <= band                    # the sandwich says something: ranks run into the thousands
    res = ops.decoder_rank(Zc.to(dev), np.stack([src, dst]), exclude_self=False)
    greater, equal = res.greater.cpu(), res.equal.cpu()
    print(f"n = {n}: max (greater - L) {int((greater - L).max())}, min (H - greater - equal) "
          f"{int((H - greater - equal).min())}, max score error / bound "
          f"{float(((res.score.cpu().double() - t).abs() / tb).max()):.3f}")
    assert bool((L <= greater).all()) and bool((greater + equal <= H).all())
    assert bool(((res.score.cpu().double() - t).abs() <= tb).all())
    assert bool((res.candidates.cpu() == n - 1).all())


# ------------------------------------------------------------------ model level: the reference's recorded logits
def _golden_sandwich(S, src, dst, ok_of, tol=1e-5):
    """K16's golden bound, tol max(1, |s|) per score (check_topk of test_gpu_decoder_topk.py), on both sides of the
    compare: L = #{S_ic - S_ij > margin}, H = #{S_ic - S_ij >= -margin}, margin = tol (max(1, |S_ic|) + max(1, |S_ij|))"""
    L, H, T = [], [], []
    for i, j in zip(src, dst):
        s = S[i]
        ok = ok_of(i).copy()
        ok[j] = False
        margin = tol * (np.maximum(1.0, np.abs(s)) + max(1.0, abs(s[j])))
        L.append(int(((s - s[j] > margin) & ok).sum()))
        H.append(int(((s - s[j] >= -margin) & ok).sum()))
        T.append(s[j])
    return np.array(L), np.array(H), np.array(T)


def _check_inside(res, L, H, T, cand, tol=1e-5):
    greater, equal = as_np(res.greater), as_np(res.equal)
    assert (L <= greater).all() and (greater + equal <= H).all()
    assert (np.abs(as_np(res.score).astype(np.float64) - T) <= tol * np.maximum(1.0, np.abs(T))).all()
    assert np.array_equal(as_np(res.candidates), cand)


def _golden_queries(g, n, rng):
    """every edge of the graph as (destination, source) -- targets inside the filtered row -- and random pairs"""
    src = np.concatenate([g["dst"].astype(np.int64), rng.integers(0, n, 300)])
    dst = np.concatenate([g["src"].astype(np.int64), rng.integers(0, n, 300)])
    return src, dst


@pytest.mark.parametrize("case", CASES)
def test_rank_links_matches_reference_logits(case, dev):
    from rank_ref import candidate_row
    g = load_golden(case)
    model = build_model(g, dev)
    gr = fresh_graph(g, dev)
    n = int(g["n"])
    src, dst = _golden_queries(g, n, np.random.default_rng(0))
    res = model.rank_links(gr, np.stack([src, dst]))
    csr = host_csr(gr)
    S = g["logits_p0"].astype(np.float64)
    L, H, T = _golden_sandwich(S, src, dst, lambda i: candidate_row(n, i, None, csr, True))
    cand = np.array([candidate_row(n, i, None, csr, True).sum() - (candidate_row(n, i, None, csr, True)[j])
                     for i, j in zip(src, dst)])
    _check_inside(res, L, H, T, cand)


def _mol8_batch(dev):
    import gae_dgl_amd as G
    parts = load_golden("mol8_parts")
    gs = []
    for i in range(int(parts["n_graphs"])):
        gr = G.DGLGraph()
        gr.add_nodes(int(parts[f"g{i}/n"])); gr.add_edges(parts[f"g{i}/src"], parts[f"g{i}/dst"])
        gr.ndata['h'] = torch.from_numpy(parts[f"g{i}/X"])
        gs.append(gr.to(dev))
    return G.batch(gs)


def test_mol8_graph_scope_matches_reference_blocks(dev):
    from rank_ref import candidate_row
    whole = load_golden("mol8")
    bg = _mol8_batch(dev)
    model = build_model(whole, dev)
    gp = as_np(bg.graph_ptr())
    n = int(whole["n"])
    member = np.searchsorted(gp, np.arange(n), side="right") - 1
    windows = np.stack([gp[member], gp[member + 1]], 1)
    csr = host_csr(bg)
    src, dst = _golden_queries(whole, n, np.random.default_rng(1))
    res = model.rank_links(bg, np.stack([src, dst]), scope="graph")
    S = whole["logits_p0"].astype(np.float64)
    rows = {i: candidate_row(n, i, windows, csr, True) for i in set(src.tolist())}
    L, H, T = _golden_sandwich(S, src, dst, lambda i: rows[i])
    cand = np.array([rows[i].sum() - rows[i][j] for i, j in zip(src, dst)])
    _check_inside(res, L, H, T, cand)
    assert (cand <= np.diff(gp).max()).all()              # candidates stay inside the molecule


def test_filter_graph_supplies_the_filtered_rows(dev):
    """filter_graph = a larger graph than the one encoded: its rows are left out, the encoder still sees g"""
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    g = load_golden("sym200")
    model = build_model(g, dev)
    n = int(g["n"])
    rng = np.random.default_rng(2)
    extra_s, extra_d = rng.integers(0, n, 400), rng.integers(0, n, 400)
    full = G.DGLGraph()
    full.add_nodes(n)
    full.add_edges(np.concatenate([g["src"], extra_s]), np.concatenate([g["dst"], extra_d]))
    full.to(dev)
    pairs = np.stack([extra_d, extra_s])                  # the held-out edges themselves: targets inside the filter
    gr = fresh_graph(g, dev)
    Z = model.encode(gr).detach()
    res = model.rank_links(fresh_graph(g, dev), pairs, filter_graph=full)
    direct = ops.decoder_rank_raw(Z, torch.as_tensor(pairs[0], device=dev), torch.as_tensor(pairs[1], device=dev),
                                  None, 0, full.csr())
    for x, y in zip(res, direct):
        assert torch.equal(x, y)
    own = model.rank_links(fresh_graph(g, dev), pairs)
    assert bool((res.candidates <= own.candidates).all()) and bool((res.candidates < own.candidates).any())


def test_vgae_rank_links_ranks_mu(dev):
    """VGAE.rank_links scores the mean mu (no noise): inside the fp64 sandwich of mu mu^T, the same on every call"""
    from gae_dgl_amd.vgae import VGAE
    from rank_ref import candidate_row
    g = load_golden("sym200")
    torch.manual_seed(0)
    model = VGAE(g["X"].shape[1], [32, 16]).to(dev)
    mu, _ = model.encode(fresh_graph(g, dev))
    n = int(g["n"])
    src, dst = _golden_queries(g, n, np.random.default_rng(3))
    gr = fresh_graph(g, dev)
    res = model.rank_links(gr, np.stack([src, dst]))
    csr = host_csr(gr)
    ok = np.stack([candidate_row(n, i, None, csr, True) for i in range(n)])
    t, tb, L, H = _sandwich(mu.detach().cpu().double(), src, dst, ok_rows=lambda ii: torch.from_numpy(ok[ii]).clone())
    greater, equal = res.greater.cpu(), res.equal.cpu()
    assert bool((L <= greater).all()) and bool((greater + equal <= H).all())
    assert bool(((res.score.cpu().double() - t).abs() <= tb).all())
    again = model.rank_links(fresh_graph(g, dev), np.stack([src, dst]))
    for x, y in zip(res, again):
        assert torch.equal(x, y)


def test_encode_side_effects_unchanged(dev):
    g = load_golden("sym200")
    model = build_model(g, dev)
    a, b = fresh_graph(g, dev), fresh_graph(g, dev)
    model.encode(a)
    model.rank_links(b, np.array([[0, 1], [2, 3]]))
    assert set(a.ndata) == set(b.ndata)
    for key in a.ndata:
        assert torch.equal(a.ndata[key], b.ndata[key])


# ------------------------------------------------------------------ NaN, infinities, indices out of range
def test_nan_inf_and_out_of_range(dev):
    from gae_dgl_amd import ops
    rng = np.random.default_rng(8)
    n, d = 500, 16
    Zi = rng.integers(-2, 3, (n, d)).astype(np.float32)
    Zi[11, 3] = np.nan                                    # every score with node 11 is NaN
    Zi[12, 0] = -np.inf                                   # s_{i,12} = -inf, +inf or NaN with the sign of z_i[0]
    Zi[12, 1:] = 0
    Zi[13, 0] = np.inf
    Zi[13, 1:] = 0
    src = rng.integers(0, n, 400).astype(np.int64)
    dst = rng.integers(0, n, 400).astype(np.int64)
    src[:8] = [11, 5, 12, 5, 13, 5, 12, 13]
    dst[:8] = [5, 11, 5, 12, 5, 13, 13, 12]
    bad = {20: (n, 3), 21: (3, n), 22: (-1, 3), 23: (3, -1), 24: (2 ** 40, 0), 25: (0, -2 ** 40), 399: (n, n)}
    for q, (s, t) in bad.items():
        src[q], dst[q] = s, t
    Z = torch.from_numpy(Zi).to(dev)
    res = ops.decoder_rank(Z, np.stack([src, dst]))
    torch.cuda.synchronize()
    ref = rank_ref(Zi, src, dst)
    assert_equal_ref(res, ref)
    score, greater, equal, cand = (as_np(x) for x in res)
    for q in bad:                                         # NaN and -1s; the neighbours' results match the reference
        assert np.isnan(score[q]) and greater[q] == equal[q] == cand[q] == -1
    # a NaN target ranks last: every candidate is ahead of it
    assert np.isnan(score[1]) and greater[1] == cand[1] > 0 and equal[1] == 0
    # the NaN row as a source: no score is a candidate
    assert cand[0] == 0 and greater[0] == 0 and equal[0] == 0
    ok = np.ones(400, dtype=bool)
    ok[list(bad)] = False
    assert (cand[ok] <= n - 2).all() and (cand[ok & ~np.isin(src, [11, 12, 13])] >= n - 5).all()


# ------------------------------------------------------------------ repeatable, schedule independent
def test_repeatable_and_split_independent(dev, tuning):
    from gae_dgl_amd import ops
    torch.manual_seed(2)
    rng = np.random.default_rng(2)
    n, d = 2708, 16
    Z = torch.randn(n, d, device=dev)
    Z[100] = Z[7]
    csr = _random_csr(rng, n, 6, hubs=(3, 77), full_rows=(5,))
    dcsr = dev_csr(csr, dev)
    gp, _ = _windows(n)
    node_ptr = torch.as_tensor(gp, device=dev)
    for m in (100, 3000):
        src = torch.as_tensor(rng.integers(0, n, m), device=dev)
        dst = torch.as_tensor(rng.integers(0, n, m), device=dev)
        for scope in (None, node_ptr):
            ref = None
            for splits in (0, 1, 2, 7, 16):
                tuning("rank_splits", splits)
                for _ in range(2):
                    res = ops.decoder_rank_raw(Z, src, dst, scope, int(np.diff(gp).max()), dcsr)
                    if ref is None:
                        ref = res
                    for x, y in zip(res, ref):
                        assert torch.equal(x, y), (m, splits)
            assert bool((ref.greater >= 0).all())


# ------------------------------------------------------------------ CLI
def test_cli_rank(tmp_path, capsys, monkeypatch):
    from gae_dgl_amd import metrics, ops
    from gae_dgl_amd import train_transductive as TT
    seen = {}
    real = ops.decoder_rank

    def spy(Z, pairs, g=None, **kw):
        seen.update(Z=Z.detach().clone(), pairs=np.asarray(pairs).copy(), filter=kw.get("filter_graph"), g=g)
        return real(Z, pairs, g, **kw)
    monkeypatch.setattr(ops, "decoder_rank", spy)
    TT.main(["--dataset", "cora", "-e", "20", "-s", str(tmp_path), "--seed", "0", "--log_every", "100", "--eval",
             "--rank"])
    text = capsys.readouterr().out
    line = [l for l in text.splitlines() if l.startswith("test MRR:")]
    assert len(line) == 1, text
    fields = dict(f.rsplit(":", 1) for f in line[0].split(" | "))
    got = TT.main.last_rank
    assert float(fields["test MRR"]) == pytest.approx(got["mrr"], abs=1e-4)
    assert float(fields["Hits@10"]) == pytest.approx(got["hits@10"], abs=1e-4)
    assert float(fields["Hits@100"]) == pytest.approx(got["hits@100"], abs=1e-4)
    assert float(fields["mean rank"]) == pytest.approx(got["mean_rank"], abs=0.06)
    assert float(fields["AUC (all non-edges)"]) == pytest.approx(got["auc"], abs=1e-4)
    assert 0.0 < got["mrr"] <= 1.0 and 0.0 <= got["auc"] <= 1.0
    # both directions of every held-out test pair, filtered with a graph that holds MORE edges than the training graph
    pairs = seen["pairs"]
    m = pairs.shape[1]
    assert got["queries"] == m and m % 2 == 0
    assert np.array_equal(pairs[:, :m // 2], pairs[::-1, m // 2:])
    full, g = seen["filter"], seen["g"]
    assert full is not None and full.number_of_edges() > g.number_of_edges()
    # dense fp64 evaluation of the model's Z: the rank of query q lies in [1 + L, 1 + H], so the MRR lies between the
    # means of 1 / (1 + H) and 1 / (1 + L)
    from rank_ref import candidate_row
    Z64 = seen["Z"].cpu().double()
    n = Z64.shape[0]
    csr = host_csr(full)
    ok = np.stack([candidate_row(n, i, None, csr, True) for i in range(n)])
    t, tb, L, H = _sandwich(Z64, pairs[0], pairs[1], ok_rows=lambda ii: torch.from_numpy(ok[ii]).clone())
    lo, hi = float((1 / (1 + H.double())).mean()), float((1 / (1 + L.double())).mean())
    print(f"MRR {got['mrr']:.6f} in [{lo:.6f}, {hi:.6f}]")
    assert lo - 1e-12 <= got["mrr"] <= hi + 1e-12
    assert float((1 + L.double()).mean()) - 1e-9 <= got["mean_rank"] <= float((1 + H.double()).mean()) + 1e-9
    # every target is a filtered edge of its source and is ranked all the same
    assert all(not ok[i, j] for i, j in zip(pairs[0], pairs[1]))
    # without --rank the output is as before: no such line
    capsys.readouterr()
    TT.main(["--dataset", "cora", "-e", "2", "-s", str(tmp_path), "--seed", "0", "--log_every", "100", "--eval"])
    assert "MRR" not in capsys.readouterr().out
