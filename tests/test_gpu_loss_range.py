"""The fp16-piece form of the symmetric fused loss kernel (bce_dense_sym_kernel, SymForm::kF16: the default from 5120
rows on, from 512 with knob bce_sym = 2) across the range of embedding values: scales far below fp16's normal range,
ordinary embeddings with a few tiny components, the band between the range guard (32768) and fp16's largest value,
NaN and inf, the workspace written by the last encoder layer's epilogue, and the fixed-capacity batch.

Every input first runs on the three-piece bf16 form (bce_s_bf16 = 2) and on the full-square kernel (bce_sym = 0),
then on the default form; all three must meet the suite's bounds against the fp64 oracle: loss within
TOL max(1, |ref|), gradient max|dZ - ref| / max|ref| < 5 TOL (no floor under max|ref|: the small rungs' gradients
are far below 1).  The inputs and tests/loss_pieces_ref.py's CPU model of the piece rounding are the same arrays."""
import functools

import numpy as np
import pytest
import torch

import loss_pieces_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = R.TOL
KNOBS = [pytest.param(n, d, bal, ri, id=f"{n}x{d}-bal{bal}-ri{ri}")
         for n, d in R.SHAPES for bal in (2, 0) for ri in (2, 4)]
FORMS = ("bf16", "square", "f16")          # the two existing forms first, the form under test last


@functools.lru_cache(maxsize=None)
def _problem(n):
    """(graph on the device, fp64 adjacency, pos_weight) of one size, built once"""
    import gae_dgl_amd as G
    from oracle import gae_oracle as O
    src, dst = R.sym_edges(n, seed=n)
    g = G.DGLGraph((src, dst), num_nodes=n).to(DEV)
    g.csr(); g.csc()
    adj = O.dense_adjacency(src, dst, n, dtype=torch.float64)
    return g, adj, O.pos_weight_of(adj), (src, dst)


_ORACLE = {}


def _oracle(n, key, Z, mask):
    """fp64 loss and dLoss/dZ of one input, computed once per (size, input name, mask) and shared by all knob settings"""
    from oracle import gae_oracle as O
    hit = _ORACLE.get((n, key))
    if hit is not None and np.array_equal(hit[2], Z) and (mask is None) == (hit[3] is None) and \
            (mask is None or np.array_equal(hit[3], mask)):
        return hit[0], hit[1]
    _, adj, pw, _ = _problem(n)
    Zt = torch.tensor(Z, dtype=torch.float64, requires_grad=True)
    mk = None if mask is None else torch.tensor(mask, dtype=torch.float64)
    ref = O.bce_with_logits_mean(O.decoder_logits(Zt, mk), adj, pw)
    ref.backward()
    _ORACLE[(n, key)] = (float(ref.detach()), Zt.grad.detach(), Z.copy(), None if mask is None else mask.copy())
    return _ORACLE[(n, key)][:2]


def _set_form(tuning, form, bal, ri):
    tuning("bce_sym_bal", bal)
    tuning("bce_sym_ri", ri)
    tuning("bce_sym", 0 if form == "square" else 2)
    tuning("bce_s_bf16", 2 if form == "bf16" else 3)


def _call(n, Z, mask=None, drawn=False, grad=True, sym=True):
    """one fused loss: (loss [cpu scalar tensor], dZ [cpu] or None, mask used [numpy] or None)"""
    from gae_dgl_amd import _lib, ops
    g = _problem(n)[0]
    Zd = torch.tensor(Z, device=DEV)
    if drawn:
        E = g.number_of_edges()
        buf = torch.empty_like(Zd)
        draws = torch.zeros(1, dtype=torch.int64, device=DEV)
        loss, dz = ops.decoder_bce_raw(Zd, buf, g.csr(), g.csc(), (n * n - E) / E, grad, dropout=(0.1, 7, 0, draws))
        torch.cuda.synchronize()
        assert int(draws) == 1
        out = (loss.reshape(()).cpu(), None if dz is None else dz.cpu(), buf.cpu().numpy())
    else:
        md = None if mask is None else torch.tensor(mask, device=DEV)
        if grad:
            Zd.requires_grad_(True)
            loss = ops.decoder_bce(Zd, md, g)
            loss.backward()
        else:
            with torch.no_grad():
                loss = ops.decoder_bce(Zd, md, g)
        torch.cuda.synchronize()
        out = (loss.detach().cpu(), Zd.grad.cpu() if grad else None, mask)
    kind = _lib.tuning_get("bce_last_kind")
    assert (kind in (2, 3)) if sym else kind == 1, f"bce_last_kind = {kind}"
    return out


def _errors(loss, dz, ref_loss, ref_grad):
    le = abs(float(loss) - ref_loss) / max(1.0, abs(ref_loss))
    ge = None if dz is None else float((dz.double() - ref_grad).abs().max() / ref_grad.abs().max())
    return le, ge


def _check(tag, loss, dz, ref_loss, ref_grad):
    le, ge = _errors(loss, dz, ref_loss, ref_grad)
    print(f"loss_range {tag}: loss err {le:.2e}" + ("" if ge is None else f", grad err {ge:.2e}"))
    assert bool(torch.isfinite(loss)) and le <= TOL, (tag, float(loss), ref_loss)
    if dz is not None:
        assert bool(torch.isfinite(dz).all()) and ge < 5 * TOL, (tag, ge)


def _all_forms(tuning, n, d, bal, ri, name, Z, mask=None, drawn=False, loss_only=True):
    """the rule of this file: the three-piece bf16 form and the full-square kernel, then the default form, each
    against the fp64 oracle in gradient mode and in loss-only mode.  Returns {form: (loss, dZ)}."""
    out = {}
    for form in FORMS:
        _set_form(tuning, form, bal, ri)
        sym = form != "square"
        loss, dz, used = _call(n, Z, mask, drawn, True, sym)
        ref_loss, ref_grad = _oracle(n, (name, "drawn" if drawn else "given" if mask is not None else "none"), Z, used)
        _check(f"{n}x{d} bal={bal} ri={ri} {name} {form}", loss, dz, ref_loss, ref_grad)
        if loss_only:
            lo, _, used2 = _call(n, Z, mask, drawn, False, sym)
            assert used is None or np.array_equal(used, used2)
            _check(f"{n}x{d} bal={bal} ri={ri} {name} {form} loss-only", lo, None, ref_loss, ref_grad)
        out[form] = (loss, dz)
    return out


@pytest.mark.parametrize("masked", ["none", "given", "drawn"])
@pytest.mark.parametrize("n,d,bal,ri", KNOBS)
def test_scale_ladder(n, d, bal, ri, masked, tuning):
    """Z = base * s down to pieces that are all zero.  The fp16 pieces of a value below 2^-14 carry an ABSOLUTE error
    of up to 2^-25, but only P V = (sigmoid(S) - 1/2) Zt runs on them: the 1/2 colsum(Zt) and edge parts of the
    gradient come from the fp32 values, and P shrinks with the logits.  Measured on an MI355X (MEASUREMENTS.md): the
    gradient error of the fp16 form is at most 2.4e-7 on every rung, the three-piece bf16 form's figure."""
    mask = R.given_mask(n, d) if masked == "given" else None
    for s in R.LADDER:
        _all_forms(tuning, n, d, bal, ri, f"ladder_{s:g}", R.ladder_input(n, d, s), mask, masked == "drawn")


@pytest.mark.parametrize("n,d,bal,ri", KNOBS)
def test_mixed_scale_stays_on_the_fp16_form(n, d, bal, ri, tuning):
    """ordinary embeddings with tiny rows, columns or entries meet the bounds ON the fp16 form: its bits differ from
    the three-piece bf16 form's, which is what a low-side guard per value would have handed them to"""
    for name, Z in R.mixed_inputs(n, d).items():
        out = _all_forms(tuning, n, d, bal, ri, name, Z, loss_only=False)
        assert not torch.equal(out["f16"][1], out["bf16"][1]), name


@pytest.mark.parametrize("n,d,bal,ri", KNOBS)
def test_guard_band(n, d, bal, ri, tuning):
    """one entry at or beyond the range guard, in a row panel's first row and in the last row (a tail tile).
    |v| = 32768 stays on the fp16 form; every |v| above it -- fp16 values up to 65504 included, where the guard and
    not an overflow has to act -- gives the three-piece bf16 form's bits; the guard re-arms after every such call"""
    plain = R.ladder_input(n, d, 1.0) * np.float32(0.7)
    _set_form(tuning, "f16", bal, ri)
    l0, g0, _ = _call(n, plain)
    for pos in R.guard_positions(n, d):
        for v in R.GUARD_IN:
            out = _all_forms(tuning, n, d, bal, ri, f"guard_{v:g}@{pos[0]}", R.guard_input(n, d, v, pos), loss_only=False)
            assert not torch.equal(out["f16"][1], out["bf16"][1]), (v, pos)
        for v in R.GUARD_OUT:
            out = _all_forms(tuning, n, d, bal, ri, f"guard_{v!r}@{pos[0]}", R.guard_input(n, d, v, pos), loss_only=False)
            assert torch.equal(out["f16"][0], out["bf16"][0]) and torch.equal(out["f16"][1], out["bf16"][1]), (v, pos)
            l1, g1, _ = _call(n, plain)                 # (the default form is still set)
            assert torch.equal(l0, l1) and torch.equal(g0, g1), (v, pos)


@pytest.mark.parametrize("n,d,bal,ri", KNOBS)
def test_non_finite_embedding_gives_a_non_finite_loss(n, d, bal, ri, tuning):
    """A NaN does not fire the range guard (fmaxf drops it): it propagates through the fp16 pieces as it does through
    the bf16 ones.  +inf fires the guard and the three-piece form turns it into NaN (inf - inf in the split).  Either
    way the loss is not finite, the poisoned row's gradient is not finite, and the next call is untouched."""
    plain = R.ladder_input(n, d, 1.0) * np.float32(0.7)
    for form in ("f16", "bf16"):
        _set_form(tuning, form, bal, ri)
        l0, g0, _ = _call(n, plain)
        for bad in (np.nan, np.inf):
            for pos in R.guard_positions(n, d):
                Z = R.guard_input(n, d, bad, pos)
                loss, dz, _ = _call(n, Z)
                assert not bool(torch.isfinite(loss)), (form, bad, pos, float(loss))
                assert not bool(torch.isfinite(dz[pos[0]]).all()), (form, bad, pos)
                assert not bool(torch.isfinite(_call(n, Z, grad=False)[0])), (form, bad, pos)     # loss-only mode
                l1, g1, _ = _call(n, plain)
                assert torch.equal(l0, l1) and torch.equal(g0, g1), (form, bad, pos)


@pytest.mark.parametrize("n,d,bal,ri", KNOBS)
def test_fixed_capacity_batch_of_small_embeddings(n, d, bal, ri, tuning):
    """gae_decoder_bce_padded (device-side counts, 77 zero-padded rows) on the 1e-5 rung against the oracle of the
    unpadded graph"""
    import gae_dgl_amd as G
    from gae_dgl_amd import _lib, ops
    src, dst = _problem(n)[3]
    Z = R.ladder_input(n, d, 1e-5)
    ref_loss, ref_grad = _oracle(n, ("ladder_1e-05", "none"), Z, None)
    cap = n + 77
    g = G.DGLGraph((src, dst), num_nodes=cap).to(DEV)
    counts = torch.tensor([n, len(src)], dtype=torch.int64, device=DEV)
    Zp = torch.zeros(cap, d, device=DEV)
    Zp[:n] = torch.tensor(Z, device=DEV)
    for form in ("bf16", "f16"):
        _set_form(tuning, form, bal, ri)
        loss, dz = ops.decoder_bce_raw(Zp, None, g.csr(), g.csc(), 0.0, True, counts=counts)
        torch.cuda.synchronize()
        assert _lib.tuning_get("bce_last_kind") in (2, 3)
        _check(f"{n}x{d} bal={bal} ri={ri} padded ladder_1e-05 {form}", loss.reshape(()).cpu(), dz[:n].cpu(), ref_loss, ref_grad)
        assert float(dz[n:].abs().max()) == 0.0


def test_small_embeddings_through_the_producer_prepared_path(tuning):
    """GAE(40, [32, 16]) whose last layer is scaled to an embedding of standard deviation 1e-4: Zt and the pieces come
    from the last layer's epilogue (gae_x_gcn_layer_fused_prep), the mask is drawn there, the symmetric fp16 form
    evaluates the loss; parameter gradients against the oracle's model in fp64 on the same mask.  The bound is
    test_gae_loss_and_grads' 5 TOL, relative to the largest entry of each gradient (they are far below 1)."""
    import gae_dgl_amd as G
    from gae_dgl_amd import _lib, ops
    from oracle import gae_oracle as O
    n = 1100
    g, _, _, (src, dst) = _problem(n)
    torch.manual_seed(5)
    X = torch.randn(n, 40, device=DEV)
    model = G.GAE(40, [32, 16]).to(DEV)
    model.decoder.seed = 13
    model.decoder.dropout = 0.1
    g.ndata['h'] = X
    with torch.no_grad():
        f = 1e-4 / float(model.encode(g).std())
        model.layers[-1].apply_mod.linear.weight.mul_(f)
        model.layers[-1].apply_mod.linear.bias.mul_(f)
    tuning("bce_sym", 2)
    g.ndata['h'] = X
    before = ops.STATS["prepared_losses"]
    loss = model.reconstruction_loss(g)
    assert ops.STATS["prepared_losses"] == before + 1, "the prepare step did not run in the last layer's epilogue"
    assert _lib.tuning_get("bce_last_kind") in (2, 3)
    ops.backward(loss, list(model.parameters()))
    torch.cuda.synchronize()
    z = g.ndata.pop('h')
    assert 0.5e-4 < float(z.std()) < 2e-4
    Ws = [l.apply_mod.linear.weight.detach().double().cpu() for l in model.layers]
    bs = [l.apply_mod.linear.bias.detach().double().cpu() for l in model.layers]
    ref_loss, ref_z, _, dW, db = O.gae_loss_and_grads(src, dst, n, X.double().cpu(), Ws, bs,
                                                      mask=model.decoder.last_mask.double().cpu())
    assert float((z.double().cpu() - ref_z).abs().max() / ref_z.abs().max()) < TOL
    assert abs(float(loss.detach()) - float(ref_loss)) <= TOL * max(1.0, abs(float(ref_loss)))
    for l, w, b in zip(model.layers, dW, db):
        for name, got, ref in (("weight", l.apply_mod.linear.weight.grad, w), ("bias", l.apply_mod.linear.bias.grad, b)):
            err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
            print(f"loss_range prepared path {name} {tuple(ref.shape)}: grad err {err:.2e}")
            assert err < 5 * TOL, (name, tuple(ref.shape), err)
