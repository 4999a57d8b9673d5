"""K17 on the GPU: gae_decoder_bce_sampled against the fused exact loss (m = N), the numpy sampler (bits), an fp64
evaluation of the estimate (arithmetic, hub rows in chunks), its expectation (unbiased), its determinism (draws, row
blocks, captured replays) and training with it (GAE, train_transductive --loss_samples)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampled_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def graph_of(n, src, dst):
    import gae_dgl_amd as G
    gr = G.DGLGraph()
    gr.add_nodes(int(n)); gr.add_edges(np.asarray(src, np.int64), np.asarray(dst, np.int64))
    return gr.to(DEV)


def counter(v=0):
    return torch.full((1,), int(v), dtype=torch.int64, device=DEV)


def pw_of(n, e):
    return (float(n) * n - e) / e


def directed_graph():
    """directed edges with duplicates and self-loops"""
    rng = np.random.default_rng(9)
    n = 150
    src = rng.integers(0, n, 700); dst = rng.integers(0, n, 700)
    src = np.concatenate([src, [4, 4, 4, 7, 7, 20]]); dst = np.concatenate([dst, [9, 9, 9, 7, 7, 20]])
    Z = rng.normal(size=(n, 12)).astype(np.float32) * 0.5
    return n, src, dst, Z


def fixture(name):
    if name == "directed":
        return directed_graph()
    g = load_golden(name)
    return int(g["n"]), g["src"], g["dst"], g["Z"].astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. exact at m = N
@pytest.mark.parametrize("name", ["tiny", "sym200", "mol8", "wide300", "directed"])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_full_cover_equals_fused_loss(name, p_drop):
    from gae_dgl_amd import ops
    n, src, dst, Zn = fixture(name)
    g = graph_of(n, src, dst)
    Z = torch.from_numpy(Zn).to(DEV)
    pw = pw_of(n, len(src))
    m_ex = torch.empty_like(Z) if p_drop else None
    m_sa = torch.empty_like(Z) if p_drop else None
    c_ex, c_sa = counter(3), counter(3)
    loss0, dZ0 = ops.decoder_bce_raw(Z, m_ex, g.csr(), g.csc(), pw, dropout=(p_drop, 77, 5, c_ex) if p_drop else None)
    loss1, dZ1, part = ops.decoder_bce_sampled_raw(Z, m_sa, g.csr(), g.csc(), pw, n, seed=77, offset=5, draws=c_sa,
                                                   dropout_p=p_drop, partners=True)
    if p_drop:
        assert torch.equal(m_ex, m_sa)                      # the same mask bits at the same draw
        assert int(c_sa) == 4
    assert rel(loss1, loss0) < 1e-5
    assert rel(dZ1, dZ0) < 1e-5
    # full cover: every ordered pair once
    assert torch.equal(part.sort(dim=1).values.cpu(), torch.arange(n).expand(n, n).int())
    # fp64 oracle
    Zt = (Z * m_sa if p_drop else Z).cpu().numpy()
    L, G = R.exact_loss(Zt, src, dst, pw)
    if p_drop:
        G = G * m_sa.cpu().numpy()
    assert rel(loss1, np.float64(L).reshape(1)) < 1e-5
    assert rel(dZ1, G) < 1e-5


def test_loss_only_and_given_mask():
    from gae_dgl_amd import ops
    n, src, dst, Zn = fixture("sym200")
    fx = load_golden("sym200")
    g = graph_of(n, src, dst)
    Z = torch.from_numpy(Zn).to(DEV)
    mask = torch.from_numpy(fx["mask"]).to(DEV)
    pw = pw_of(n, len(src))
    l0, _ = ops.decoder_bce_raw(Z, mask, g.csr(), None, pw, want_grad=False)
    l1, d1, _ = ops.decoder_bce_sampled_raw(Z, mask, g.csr(), None, pw, n, want_grad=False)
    assert d1 is None and rel(l1, l0) < 1e-5
    # the reference's own value (the fixture's p01 loss was computed with this mask)
    assert rel(l1, np.float64(fx["loss_p01"]).reshape(1)) < 1e-5


# ------------------------------------------------------------------------------------------ 2. sampler bits
@pytest.mark.parametrize("n,m,seed,draw,offset", [(1, 1, 0, 0, 0), (2, 2, 1, 5, 0), (3, 2, 9, 0, 3), (1024, 7, 5, 1, 0),
                                                  (1025, 16, 5, 2, 7), (4096, 64, 123, 1 << 33, 1),
                                                  (19717, 8, 42, 3, 0), ((1 << 16) + 1, 5, 2, 11, 2)])
def test_partners_match_numpy(n, m, seed, draw, offset):
    from gae_dgl_amd import ops
    Z = torch.randn(n, 4, device=DEV)
    ip = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    ix = torch.zeros(1, dtype=torch.int32, device=DEV)
    c = counter(draw)
    _, _, part = ops.decoder_bce_sampled_raw(Z, None, (ip, ix), (ip, ix), 1.0, m, seed=seed, offset=offset, draws=c,
                                             partners=True)
    assert int(c) == draw + 1
    want = R.partners(seed, offset + draw, n, m, np.arange(n))
    assert np.array_equal(part.cpu().numpy(), want)


def test_partners_match_numpy_at_2_24_rows_form():
    from gae_dgl_amd import ops
    n, m, r0, nl = 1 << 24, 16, 0, 4096
    Z = torch.zeros(n, 4, device=DEV)
    ip = torch.zeros(nl + 1, dtype=torch.int32, device=DEV)
    ix = torch.zeros(1, dtype=torch.int32, device=DEV)
    for seed, draw in ((0, 0), (31, 1000)):
        _, _, part = ops.decoder_bce_sampled_raw(Z, None, (ip, ix), (ip, ix), 1.0, m, seed=seed, draws=counter(draw),
                                                 row_begin=r0, n_local=nl, partners=True)
        assert np.array_equal(part.cpu().numpy(), R.partners(seed, draw, n, m, np.arange(r0, r0 + nl)))
    # a block further down
    _, _, part = ops.decoder_bce_sampled_raw(Z, None, (ip, ix), (ip, ix), 1.0, m, seed=3, draws=counter(2),
                                             row_begin=n - nl, n_local=nl, partners=True)
    assert np.array_equal(part.cpu().numpy(), R.partners(3, 2, n, m, np.arange(n - nl, n)))


# ------------------------------------------------------------------------------------------ 3. arithmetic
def check_against_fp64(Z, csr, csc, pw, m, seed, draw, r0, nl, n_edges_hint=None):
    from gae_dgl_amd import ops
    dev_csr = tuple(torch.from_numpy(a).to(DEV) for a in csr)
    dev_csc = tuple(torch.from_numpy(a).to(DEV) for a in csc)
    loss, dZ, part = ops.decoder_bce_sampled_raw(Z, None, dev_csr, dev_csc, pw, m, seed=seed, draws=counter(draw),
                                                 row_begin=r0, n_local=nl, partners=True)
    Zn = Z.cpu().numpy()
    L, G = R.estimate(Zn, csr, csc, pw, seed, draw, m, r0, nl, part=part.cpu().numpy().astype(np.int64))
    assert np.array_equal(part.cpu().numpy(), R.partners(seed, draw, Z.shape[0], m, np.arange(r0, r0 + nl)))
    assert rel(loss, np.float64(L).reshape(1)) < 1e-5
    assert rel(dZ, G) < 1e-5
    return loss, dZ


def test_arithmetic_pubmed_planetoid_m8():
    from gae_dgl_amd import workloads as W
    n, src, dst, _ = W.citation_graph("pubmed", degrees="planetoid")
    gen = torch.Generator(device=DEV).manual_seed(1)
    Z = torch.randn(n, 16, device=DEV, generator=gen) * 0.3
    csr, csc = R.csr_of(dst, src, n), R.csr_of(src, dst, n)
    check_against_fp64(Z, csr, csc, pw_of(n, len(src)), 8, 7, 2, 0, n)


def test_arithmetic_heavy_rows_in_chunks():
    """a hub whose pair list (in + out edges + 2 m samples) spans several 4096-pair chunks, beside light rows"""
    rng = np.random.default_rng(4)
    n = 6000
    hub = np.arange(1, n)
    src = np.concatenate([hub, np.zeros(n - 1, np.int64), rng.integers(0, n, 20000), [5] * 5000])
    dst = np.concatenate([np.zeros(n - 1, np.int64), hub, rng.integers(0, n, 20000), [9] * 5000])   # 5 -> 9 x 5000
    Z = torch.from_numpy(rng.normal(size=(n, 16)).astype(np.float32) * 0.2).to(DEV)
    pw = pw_of(n, len(src))
    check_against_fp64(Z, R.csr_of(dst, src, n), R.csr_of(src, dst, n), pw, 32, 1, 0, 0, n)
    check_against_fp64(Z, R.csr_of(dst, src, 700, 0), R.csr_of(src, dst, 700, 0), pw, 32, 1, 0, 0, 700)


def test_arithmetic_rmat_s24_rows_m16():
    from gae_dgl_amd import workloads as W
    scale, nl = 24, 4000
    n = 1 << scale
    src, dst = W.rmat_edges(scale, 16, seed=0, device=DEV)
    E = int(src.numel())
    rows_a = dst < nl
    rows_t = src < nl
    a_r, a_c = dst[rows_a].cpu().numpy(), src[rows_a].cpu().numpy()
    t_r, t_c = src[rows_t].cpu().numpy(), dst[rows_t].cpu().numpy()
    del src, dst, rows_a, rows_t
    torch.cuda.empty_cache()
    csr, csc = R.csr_of(a_r, a_c, nl), R.csr_of(t_r, t_c, nl)
    assert np.diff(csr[0]).max() + np.diff(csc[0]).max() > 4 * 4096     # hub rows: several chunks each
    gen = torch.Generator(device=DEV).manual_seed(2)
    Z = torch.randn(n, 16, device=DEV, generator=gen) * 0.05
    check_against_fp64(Z, csr, csc, pw_of(n, E), 16, 5, 1, 0, nl)


# ------------------------------------------------------------------------------------------ 4. unbiased
def planted_partition(n, k, p_in, p_out, seed):
    rng = np.random.default_rng(seed)
    comm = np.arange(n) % k
    iu = np.triu_indices(n, 1)
    same = comm[iu[0]] == comm[iu[1]]
    keep = rng.random(iu[0].size) < np.where(same, p_in, p_out)
    a, b = iu[0][keep], iu[1][keep]
    return np.concatenate([a, b]), np.concatenate([b, a]), comm


def test_unbiased_over_draws():
    from gae_dgl_amd import ops
    n, d, m, draws = 500, 4, 4, 2000
    src, dst, _ = planted_partition(n, 5, 0.05, 0.004, 0)
    g = graph_of(n, src, dst)
    rng = np.random.default_rng(1)
    Z = torch.from_numpy(rng.normal(size=(n, d)).astype(np.float32) * 0.6).to(DEV)
    pw = pw_of(n, len(src))
    L, G = ops.decoder_bce_raw(Z, None, g.csr(), g.csc(), pw)
    c = counter(0)
    s1 = torch.zeros((), dtype=torch.float64, device=DEV); s2 = torch.zeros_like(s1)
    g1 = torch.zeros(n, d, dtype=torch.float64, device=DEV); g2 = torch.zeros_like(g1)
    for _ in range(draws):
        l, dz, _ = ops.decoder_bce_sampled_raw(Z, None, g.csr(), g.csc(), pw, m, seed=17, draws=c)
        l = l.double()[0]; dz = dz.double()
        s1 += l; s2 += l * l; g1 += dz; g2 += dz * dz
    assert int(c) == draws
    mean = float(s1) / draws
    se = np.sqrt(max(float(s2) / draws - mean ** 2, 0.0) / (draws - 1))
    assert abs(mean - float(L)) < 4 * se, (mean, float(L), se)
    gm = g1 / draws
    gse = ((g2 / draws - gm ** 2).clamp(min=0) / (draws - 1)).sqrt()
    z = ((gm - G.double()).abs() / gse.clamp(min=1e-30)).cpu().numpy()
    assert z.max() < 4.0, (z.max(), int((z > 4).sum()))


# ------------------------------------------------------------------------------------------ 5. deterministic
def hub_graph():
    rng = np.random.default_rng(12)
    n = 5000
    hub = np.arange(1, 4500)
    src = np.concatenate([hub, np.zeros(hub.size, np.int64), rng.integers(0, n, 30000)])
    dst = np.concatenate([np.zeros(hub.size, np.int64), hub, rng.integers(0, n, 30000)])
    return n, src, dst


def test_same_draw_same_bits_and_row_blocks():
    from gae_dgl_amd import ops
    n, src, dst = hub_graph()
    g = graph_of(n, src, dst)
    gen = torch.Generator(device=DEV).manual_seed(8)
    Z = torch.randn(n, 16, device=DEV, generator=gen) * 0.3
    pw = pw_of(n, len(src))
    mk = lambda: torch.empty_like(Z)                                    # noqa: E731
    m1 = mk()
    l1, d1, _ = ops.decoder_bce_sampled_raw(Z, m1, g.csr(), g.csc(), pw, 12, seed=4, draws=counter(6), dropout_p=0.2)
    m2 = mk()
    l2, d2, _ = ops.decoder_bce_sampled_raw(Z, m2, g.csr(), g.csc(), pw, 12, seed=4, draws=counter(6), dropout_p=0.2)
    assert torch.equal(l1, l2) and torch.equal(d1, d2) and torch.equal(m1, m2)
    l3, _, _ = ops.decoder_bce_sampled_raw(Z, mk(), g.csr(), g.csc(), pw, 12, seed=4, draws=counter(7), dropout_p=0.2)
    assert not torch.equal(l1, l3)
    ip, ix = g.csr(); tp, tx = g.csc()
    for blocks in (1, 2, 7):
        bounds = np.linspace(0, n, blocks + 1).astype(np.int64)
        bounds[1:-1] += 3                                               # (not multiples of any tile)
        tot, parts = 0.0, []
        for r0, r1 in zip(bounds[:-1], bounds[1:]):
            r0, r1 = int(r0), int(r1)
            lb, db, _ = ops.decoder_bce_sampled_raw(Z, m1, (ip[r0:r1 + 1], ix), (tp[r0:r1 + 1], tx), pw, 12, seed=4,
                                                    draws=counter(6), row_begin=r0, n_local=r1 - r0)
            tot += float(lb.double()); parts.append(db)
        assert torch.equal(torch.cat(parts), d1), blocks
        assert abs(tot - float(l1.double())) <= 1e-6 * abs(float(l1.double()))


def make_model(in_dim, seed=0):
    import gae_dgl_amd as G
    torch.manual_seed(seed)
    return G.GAE(in_dim, [32, 16]).to(DEV)


def test_captured_replays_equal_eager_steps():
    from gae_dgl_amd import ops
    from gae_dgl_amd.capture import CapturedTrainStep
    from gae_dgl_amd.optim import Adam
    n, src, dst = hub_graph()
    g = graph_of(n, src, dst)
    X = torch.randn(n, 24, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    k = 8
    m_eager = make_model(24)
    m_cap = copy.deepcopy(m_eager)
    m_eager.decoder.seed = m_cap.decoder.seed = 21
    o_eager, o_cap = Adam(m_eager.parameters(), lr=1e-2), Adam(m_cap.parameters(), lr=1e-2)
    eager = []
    for _ in range(5):
        g.ndata['h'] = X
        loss = m_eager.reconstruction_loss(g, samples=k)
        o_eager.zero_grad()
        ops.backward(loss)
        o_eager.step()
        eager.append(loss.detach().clone())
    step = CapturedTrainStep(m_cap, o_cap, g, X, loss_fn=lambda mm, gg: mm.reconstruction_loss(gg, samples=k), warmup=0)
    cap = [step().clone() for _ in range(5)]
    assert all(torch.equal(a, b) for a, b in zip(eager, cap)), (eager, cap)
    assert len({float(v) for v in eager}) == 5                            # the counter advances: new pairs each step
    for (ka, a), (kb, b) in zip(m_eager.state_dict().items(), m_cap.state_dict().items()):
        assert torch.equal(a, b), ka
    assert int(m_cap.decoder._draws) == 5


def test_sharded_rows_match_one_gpu():
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from gae_dgl_amd.parallel import LocalGroup, ShardedGraph
    n, src, dst = hub_graph()
    srct, dstt = torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(3)
    Z = torch.randn(n, 16, device=DEV, generator=gen) * 0.4
    mask = ops.dropout_mask((n, 16), 0.1, seed=5, device=DEV)
    g = G.DGLGraph((srct, dstt), num_nodes=n).to(DEV)
    Z0 = Z.clone().requires_grad_(True)
    ref = ops.decoder_bce_sampled(Z0, mask, g, 6, dropout=(0.0, 0, 0, counter(0)))
    ref.backward()
    world = 3
    grp = LocalGroup(world)
    grp.publish(Z * mask)
    total, grads = 0.0, []
    for r in range(world):
        sg = ShardedGraph(n, srct, dstt, rank=r, group=grp, device=DEV)
        p = sg.part
        z = Z[p.r0:p.r1].clone().requires_grad_(True)
        part = ops.sharded_decoder_bce_sampled(z, mask[p.r0:p.r1], sg, 6, n_edges_global=len(src))
        part.backward()
        assert int(sg._loss_draws) == 1
        total += float(part.detach()); grads.append(z.grad)
    assert abs(total - float(ref.detach())) < 1e-6 * abs(float(ref.detach()))
    assert rel(torch.cat(grads), Z0.grad) < 1e-6


# ------------------------------------------------------------------------------------------ 6. it trains
def test_sampled_training_matches_exact_training(capsys):
    import gae_dgl_amd as G
    from gae_dgl_amd import metrics, ops
    from gae_dgl_amd.optim import Adam
    n = 2000
    src, dst, comm = planted_partition(n, 8, 0.03, 0.0015, 5)
    kept, val, test = metrics.split_edges(src, dst, n, seed=0)
    g = G.DGLGraph(kept, num_nodes=n).to(DEV)
    rng = np.random.default_rng(2)
    X = torch.from_numpy((np.eye(8)[comm] + rng.normal(size=(n, 8)) * 1.0).astype(np.float32)).to(DEV)
    X = torch.cat([X, torch.from_numpy(rng.normal(size=(n, 24)).astype(np.float32)).to(DEV)], 1)
    results = {}
    for samples in (None, 8):
        model = make_model(32, seed=1)
        model.decoder.seed = 3
        opt = Adam(model.parameters(), lr=1e-2)
        for _ in range(200):
            g.ndata['h'] = X
            loss = model.reconstruction_loss(g, samples=samples)
            opt.zero_grad()
            ops.backward(loss)
            opt.step()
        model.decoder.dropout = 0.0
        g.ndata['h'] = X
        with torch.no_grad():
            exact = float(model.reconstruction_loss(g))
            g.ndata['h'] = X
            Z = model.encode(g)
        results[samples] = (exact, metrics.evaluate(Z, test)["auc"])
    (le, ae), (ls, as_) = results[None], results[8]
    with capsys.disabled():
        print(f"\n[sampled training] exact-trained: loss {le:.5f} AUC {ae:.4f} | m = 8: loss {ls:.5f} AUC {as_:.4f}")
    assert ls <= 1.05 * le, (ls, le)
    assert abs(as_ - ae) <= 0.02, (as_, ae)


# ------------------------------------------------------------------------------------------ 7. the CLI
def test_train_transductive_loss_samples_eager_equals_captured(tmp_path):
    from gae_dgl_amd import train_transductive as TT
    base = ["--dataset", "cora", "-e", "12", "-s", str(tmp_path), "--seed", "0", "--log_every", "100", "--eval",
            "--loss_samples", "8"]
    captured = TT.main(base)
    auc = TT.main.last_eval["auc"]
    eager = TT.main(base + ["--no_hipgraph"])
    assert captured == eager
    assert len(set(captured)) > 1
    assert 0.0 <= auc <= 1.0 and TT.main.last_eval["auc"] == auc
