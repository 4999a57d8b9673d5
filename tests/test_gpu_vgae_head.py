"""gae_vgae_head_fwd / gae_vgae_head_bwd / gae_x_vgae_head_prep through the raw C ABI, and the three autograd surfaces on
top of them, against tests/noise_ref.py (float64, a derived rounding bound per element).  Every call's operands sit in
one dense_ref.Arena: NaN guards around each operand, NaN pad columns [d, ldm), a workspace of exactly the queried size.

Shapes: (1, 1); (63, 3) / (64, 16) / (65, 17) around the 64-row block and the 4-wide vectors; (257, 64) more than one
thread block; (4101, 64) = 262 464 elements, above the 1024 x 256 threads a launch has, so the stride loop runs twice.
Layouts: ldm = d, ldm = d + 3, and packed [mu | log sigma] with ldm = 2 d.  Value regimes: (a) N(0, 0.01^2), where the KL
bracket cancels; (b) N(0, 1); (c) log sigma uniform in [-8, 8], mu uniform in [-30, 30] (exp(16) stays finite in fp32).
Lines starting with RATIO / KLREL carry the figures MEASUREMENTS.md quotes."""
import ctypes

import numpy as np
import pytest
import torch

import noise_ref as R
import vgae_abi as A

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (63, 3), (64, 16), (65, 17), (257, 64), (4101, 64)]
LAYOUTS = ["ldm=d", "ldm=d+3", "packed"]
REGIMES = ["a", "b", "c"]


def inputs(regime, n, d, seed):
    """(mu, ls, eps, dz) fp32: eps from the restated noise, dz ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    if regime == "a":
        mu, ls = (rng.standard_normal((n, d)) * 0.01 for _ in range(2))
    elif regime == "b":
        mu, ls = (rng.standard_normal((n, d)) for _ in range(2))
    else:
        ls, mu = rng.uniform(-8, 8, (n, d)), rng.uniform(-30, 30, (n, d))
    eps = R.normal_noise(n * d, A.SEED, 0, seed)[0].reshape(n, d)
    return [x.astype(np.float32) for x in (mu, ls, eps, rng.standard_normal((n, d)))]


def within(what, name, got, ref, bound, regime=None):
    ratio, at = R.worst(got, ref, bound)
    print(f"RATIO regime={regime} tensor={name} ratio={ratio:.4f} ({what}, element {at})")
    assert ratio <= 1.0, (what, name, ratio, at, np.asarray(got).reshape(-1)[at], np.asarray(ref).reshape(-1)[at],
                          np.broadcast_to(bound, np.shape(ref)).reshape(-1)[at])


def head_arena(n, d, layout, mu, ls, eps, dz, gkl, ws_bytes):
    a = A.arena()
    if layout == "packed":
        a.add("ml", n, 2 * d, 2 * d, 0, np.concatenate([mu, ls], 1)).add("dml", n, 2 * d, 2 * d)
    else:
        ldm = d if layout == "ldm=d" else d + 3
        a.add("mu", n, d, ldm, 0, mu).add("ls", n, d, ldm, 0, ls).add("dmu", n, d, ldm).add("dls", n, d, ldm)
    a.add("eps", n, d, d, 0, eps).add("z", n, d).add("kl", 1, 1)
    if dz is not None:
        a.add("dz", n, d, d, 0, dz)
    if gkl is not None:
        a.add("gkl", 1, 1, None, 0, np.array([gkl], np.float32))
    a.add_workspace("ws", ws_bytes)
    return A.Device(a.build())


def head_pointers(dv, d, layout):
    """(mu, ls, ldm, dmu, dls, input names, gradient names)"""
    if layout == "packed":
        return dv.ptr("ml"), dv.ptr("ml", d), 2 * d, dv.ptr("dml"), dv.ptr("dml", d), ["ml"], ["dml"]
    return dv.ptr("mu"), dv.ptr("ls"), dv.a.ld("mu"), dv.ptr("dmu"), dv.ptr("dls"), ["mu", "ls"], ["dmu", "dls"]


def gradients(dv, d, layout):
    if layout == "packed":
        g = dv.a.get("dml")
        return g[:, :d], g[:, d:]
    return dv.a.get("dmu"), dv.a.get("dls")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_head_forward_and_backward(n, d, layout):
    L = A.lib()
    ws_bytes = int(L.gae_vgae_head_workspace_bytes(n * d))
    assert ws_bytes >= 8192
    for k, regime in enumerate(REGIMES):
        what = f"n={n} d={d} {layout} regime {regime}"
        mu, ls, eps, dz = inputs(regime, n, d, 10 * n + d + k)
        gkl = None if regime == "a" else 0.37                          # NULL = 1
        no_dz = regime == "c" and layout == "ldm=d+3"                   # dz = NULL (= 0) once per shape
        dv = head_arena(n, d, layout, mu, ls, eps, None if no_dz else dz, gkl, ws_bytes)
        pm, pl, ldm, pdm, pdl, ins, outs = head_pointers(dv, d, layout)
        with torch.cuda.device(A.DEV):
            rc = L.gae_vgae_head_fwd(pm, pl, ldm, dv.ptr("eps"), n, d, dv.ptr("z"), dv.ptr("kl"), dv.ptr("ws"), ws_bytes,
                                     A.stream())
            assert rc == 0, (what, rc, L.gae_last_error())
            rc = L.gae_vgae_head_bwd(None if no_dz else dv.ptr("dz"), pm, pl, ldm, dv.ptr("eps"),
                                     None if gkl is None else dv.ptr("gkl"), n, d, pdm, pdl, A.stream())
            assert rc == 0, (what, rc, L.gae_last_error())
        dv.download()
        dv.check_memory(what, ins + ["eps"] + ([] if no_dz else ["dz"]) + ([] if gkl is None else ["gkl"]),
                        ["z", "kl"] + outs)
        z, kl, zb, klb = R.head_fwd(mu, ls, eps)
        within(what, "z", dv.a.get("z"), z, zb, regime)
        got_kl = float(dv.a.get("kl")[0, 0])
        within(what, "kl", [got_kl], [kl], [klb], regime)
        print(f"KLREL regime={regime} n={n} d={d} rel={abs(got_kl - kl) / abs(kl):.3e} bound={klb / abs(kl):.3e}")
        dmu, dls, (bm, bl) = R.head_bwd(None if no_dz else dz, mu, ls, eps, None if gkl is None else np.float32(gkl), n)
        gm, gl = gradients(dv, d, layout)
        within(what, "dmu", gm, dmu, bm, regime)
        within(what, "dlogstd", gl, dls, bl, regime)


PREP_N = [1, 63, 64, 65, 130]


@pytest.mark.parametrize("draw_eps", [0, 1])
@pytest.mark.parametrize("ldm", [16, 20, 32])
@pytest.mark.parametrize("n", PREP_N)
def test_head_prep(n, ldm, draw_eps):
    L = A.lib()
    d, blocks = 16, (n + 63) // 64
    offset, draw = 3, (1 << 32) + 9
    ws_bytes = int(L.gae_vgae_head_workspace_bytes(n * d))
    for k, regime in enumerate(REGIMES):
        what = f"prep n={n} ldm={ldm} draw_eps={draw_eps} regime {regime}"
        mu, ls, eps, _ = inputs(regime, n, d, 100 * n + ldm + k)
        a = A.arena()
        if ldm == 32:
            a.add("ml", n, 32, 32, 0, np.concatenate([mu, ls], 1))
        else:
            a.add("mu", n, d, ldm, 0, mu).add("ls", n, d, ldm, 0, ls)
        a.add("eps", n, d, d, 0, None if draw_eps else eps).add("z", n, d).add("z2", n, d).add("kl2", 1, 1)
        a.add_workspace("klp", 8 * blocks).add_workspace("ws", ws_bytes)
        dv = A.Device(a.build())
        pm, pl = (dv.ptr("ml"), dv.ptr("ml", d)) if ldm == 32 else (dv.ptr("mu"), dv.ptr("ls"))
        w, dd, nb = A.PrepWorkspace(n), A.draw_tensor(draw), ctypes.c_int64(-1)
        with torch.cuda.device(A.DEV):
            rc = L.gae_x_vgae_head_prep(pm, pl, ldm, dv.ptr("eps"), draw_eps, A.SEED, offset, A.ptr(dd), n, d, dv.ptr("z"),
                                        ctypes.byref(w.lay), dv.ptr("klp"), blocks, ctypes.byref(nb), A.stream())
            assert rc == 0, (what, rc, L.gae_last_error())
            rc = L.gae_vgae_head_fwd(pm, pl, ldm, dv.ptr("eps"), n, d, dv.ptr("z2"), dv.ptr("kl2"), dv.ptr("ws"), ws_bytes,
                                     A.stream())
            assert rc == 0, (what, rc, L.gae_last_error())
        dv.download()
        ins = ["ml"] if ldm == 32 else ["mu", "ls"]
        dv.check_memory(what, ins + ([] if draw_eps else ["eps"]), ["z", "z2", "kl2"] + (["eps"] if draw_eps else []))
        assert nb.value == blocks, (what, nb.value)
        got_eps = dv.a.get("eps")
        if draw_eps:
            ref, bound = R.normal_noise(n * d, A.SEED, offset, draw)
            within(what, "eps", got_eps.reshape(-1), ref, bound, regime)
        P = R.head_prep(mu, ls, got_eps)
        zg = dv.a.get("z")
        within(what, "z", zg, P["z"], P["z_bound"], regime)
        assert np.array_equal(zg.view(np.uint32), dv.a.get("z2").view(np.uint32)), (what, "z != gae_vgae_head_fwd's z")
        out = w.read()
        assert out["clean"], (what, "written past row n / block ceil(n / 64) of the loss workspace")
        assert np.array_equal(out["Zt"].view(np.uint32), zg.view(np.uint32)), (what, "Zt != z")
        hi, lo = R.bf16_split(zg)
        assert np.array_equal(out["Zhi"], hi) and np.array_equal(out["Zlo"], lo), (what, "bf16 split")
        sums, sb = R.block_colsums(zg)
        assert np.array_equal(out["colsum"][:, 0].view(np.uint64), out["colsum"][:, 1].view(np.uint64)), (what, "copies")
        within(what, "colsum", out["colsum"][:, 0], sums, sb, regime)
        klp = dv.f64("klp")
        within(what, "kl_partial", klp, P["kl_partial"], P["kl_partial_bound"], regime)
        within(what, "kl(partials)", [klp.sum() * (-0.5 / (float(n) * float(n)))], [P["kl"]], [P["kl_bound"]], regime)
        within(what, "kl(fwd)", [float(dv.a.get("kl2")[0, 0])], [P["kl"]], [P["kl_bound"]], regime)


# ---------------------------------------------------------------------------------------------- autograd surfaces
def _fp64_grads(mu, ls, eps, w, gkl, rec=None):
    """torch fp64 autograd on the CPU: gradients of gkl * kl + sum(z w) (+ gkl * rec(z)) with respect to mu and log
    sigma; also z, kl, rec and d rec / d z"""
    n = mu.shape[0]
    tm, tl = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (mu, ls))
    z = tm + torch.tensor(eps, dtype=torch.float64) * torch.exp(tl)
    z.retain_grad()
    kl = -0.5 / n ** 2 * (1 + 2 * tl - tm ** 2 - torch.exp(2 * tl)).sum()
    total = gkl * kl + (z * torch.tensor(w, dtype=torch.float64)).sum()
    r = None
    if rec is not None:
        r = rec(z)
        total = total + gkl * r
    total.backward()
    return tm.grad.numpy(), tl.grad.numpy(), z.detach().numpy(), float(kl.detach()), r, z.grad.numpy()


def _surface_inputs():
    n, d = 130, 16
    mu, ls, eps, w = inputs("b", n, d, 77)
    return n, d, mu, ls, eps, w, float(np.float32(0.7))


def _check_surface(what, n, mu, ls, eps, w, gkl, got_z, got_kl, got_dmu, got_dls):
    rm, rl, z64, kl64, _, _ = _fp64_grads(mu, ls, eps, w, gkl)
    z, kl, zb, klb = R.head_fwd(mu, ls, eps)
    assert np.allclose(z, z64, rtol=1e-13, atol=0) and abs(kl - kl64) <= 1e-13 * abs(kl)
    _, _, (bm, bl) = R.head_bwd(w, mu, ls, eps, gkl, n)
    within(what, "z", got_z, z64, zb, "b")
    within(what, "kl", [got_kl], [kl64], [klb], "b")
    within(what, "dmu", got_dmu, rm, bm, "b")
    within(what, "dlogstd", got_dls, rl, bl, "b")


def test_autograd_vgae_head():
    from gae_dgl_amd import ops
    n, d, mu, ls, eps, w, gkl = _surface_inputs()
    tm, tl = (torch.tensor(x, device=A.DEV, requires_grad=True) for x in (mu, ls))
    z, kl = ops.vgae_head(tm, tl, torch.tensor(eps, device=A.DEV))
    (0.7 * kl + (z * torch.tensor(w, device=A.DEV)).sum()).backward()
    _check_surface("ops.vgae_head", n, mu, ls, eps, w, gkl, z.detach().cpu().numpy(), float(kl.detach()), tm.grad.cpu().numpy(),
                   tl.grad.cpu().numpy())


def test_autograd_vgae_head_packed():
    from gae_dgl_amd import ops
    n, d, mu, ls, eps, w, gkl = _surface_inputs()
    ml = torch.tensor(np.concatenate([mu, ls], 1), device=A.DEV, requires_grad=True)
    z, kl = ops.vgae_head_packed(ml, torch.tensor(eps, device=A.DEV))
    (0.7 * kl + (z * torch.tensor(w, device=A.DEV)).sum()).backward()
    g = ml.grad.cpu().numpy()
    _check_surface("ops.vgae_head_packed", n, mu, ls, eps, w, gkl, z.detach().cpu().numpy(), float(kl.detach()), g[:, :d], g[:, d:])


def test_autograd_vgae_head_loss():
    """only the loss = rec + kl carries a gradient here, so the objective is 0.7 loss: the head's backward then gets
    gkl = 0.7 and dz = 0.7 d rec / d z from the fused loss.  The head's share is held to head_bwd's bounds; the dz it is
    handed is the fused loss's gradient, which that kernel's own range test (test_gpu_loss_range._check) holds to 5e-5
    of the gradient's largest entry -- that allowance enters dmu as it is and dlogstd times |eps| exp(log sigma).  rec
    itself: against oracle.bce_with_logits_mean at 2e-5, as test_vgae_matches_oracle holds it."""
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    from oracle import gae_oracle as O
    n, d, mu, ls, eps, _, gkl = _surface_inputs()
    rng = np.random.default_rng(5)
    s, t = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    src, dst = np.concatenate([s, t]), np.concatenate([t, s])
    g = G.DGLGraph((src, dst), num_nodes=n).to(A.DEV)
    ml = torch.tensor(np.concatenate([mu, ls], 1), device=A.DEV, requires_grad=True)
    out = ops.vgae_head_loss(ml, g, eps=torch.tensor(eps, device=A.DEV))
    assert out is not None
    loss, z, kl, rec, eps_out = out
    (0.7 * loss).backward()
    torch.cuda.synchronize()
    assert torch.equal(eps_out.cpu(), torch.tensor(eps))
    adj = O.dense_adjacency(src, dst, n, dtype=torch.float64)
    pw = O.pos_weight_of(adj)
    rm, rl, z64, kl64, rec64, dz64 = _fp64_grads(mu, ls, eps, np.zeros_like(mu), gkl,
                                                 rec=lambda zz: O.bce_with_logits_mean(zz @ zz.t(), adj, pw))
    rec64 = float(rec64.detach())
    _, _, zb, klb = R.head_fwd(mu, ls, eps)
    within("ops.vgae_head_loss", "z", z.cpu().numpy(), z64, zb, "b")
    within("ops.vgae_head_loss", "kl", [float(kl)], [kl64], [klb], "b")
    rec_err = abs(float(rec) - rec64) / max(1.0, abs(rec64))
    print(f"vgae_head_loss: rec {float(rec):.6f} (fp64 {rec64:.6f}), error {rec_err:.2e}")
    assert rec_err < 2e-5
    assert abs(float(loss.detach()) - (rec64 + kl64)) < 2e-5 * max(1.0, abs(rec64 + kl64))
    _, _, (bm, bl) = R.head_bwd(dz64, mu, ls, eps, gkl, n)
    allow = 5e-5 * np.abs(dz64).max()
    gm = ml.grad.cpu().numpy()
    within("ops.vgae_head_loss", "dmu", gm[:, :d], rm, bm + allow, "b")
    within("ops.vgae_head_loss", "dlogstd", gm[:, d:], rl,
           bl + allow * np.abs(eps.astype(np.float64)) * np.exp(ls.astype(np.float64)), "b")
