"""The dense loss chain -- gae_decoder_dense, gae_csr_to_dense, gae_bce_logits, gae_decoder_dense_bwd (csrc/dense.hip,
csrc/csr_build.hip, csrc/bce_dense.hip) -- through the raw C ABI against tests/dense_loss_ref.py, in the arenas of
tests/dense_ref.py: NaN guards of 64 floats around each operand, NaN pad columns [width, ld), bases 0 or 1 float past a
16-byte boundary, a workspace of exactly the queried size.  Every case makes ONE call on the current stream and asserts:
status 0; dense_last_kind == the kind the case was built for (decoder calls); every output element within its derived
bound of float64 (no bound was widened, see MEASUREMENTS.md "Dense loss chain in guarded arenas"); the loss within its
bound; guards intact; inputs bit-unchanged, pads included; output pads still the pattern; no NaN in an output.

kind -> cases (ids of dense_loss_ref.FWD / BWD; test_dense_loss_ref_cpu.py asserts the restated dispatch agrees):
  tiled        every gae_decoder_dense call: gemm_kernel<4, bt, mul_mask, mask_b> with A = B = Z, and its unmasked form
  atb_narrow   backward with n <= 32
  atb_bf16     backward with d <= 32 < n and rows of G that are whole 16-byte vectors (132 nodes; 129 on ld 132: the
               column tail over NaN pads; 257 on ld 260: three slots); the knob at 1 and at 2
  atb_vec      the same rows of G with d > 32, or the knob at 0
  atb_scalar   any other G (129 or 131 contiguous nodes, a base one float off)
Every backward case runs with and without a mask: term 1 is gemm_kernel<1|2|4, bt=0, mask_b=1> with one,
gemm_stream_kernel or gemm_kernel<4> without."""
import numpy as np
import pytest
import torch

import dense_loss_ref as L
import dense_ref as R
from test_gpu_dense_abi import DEV, E_NULL, E_SIZE, E_WORKSPACE, Device, _kind, _stream, _within

pytestmark = pytest.mark.gpu


def _lib():
    from gae_dgl_amd import _lib
    return _lib.load()


# ---------------------------------------------------------------------------------------------- gae_decoder_dense
def _fwd_arena(c):
    n, d = c["n"], c["d"]
    Z, mask, _ = L.decoder_inputs(n, d)
    ldz = R.lead(d, c["ld_Z"])
    a = R.Arena()
    a.add("Z", n, d, ldz, c["mis_Z"], Z)
    if c["mask"]:
        a.add("mask", n, d, ldz, c["mis_m"], mask)            # the ABI has ONE ldz for both
    a.add("out", n, n, R.lead(n, c["ld_out"]), c["mis_out"])
    return a.build(), Z, (mask if c["mask"] else None)


def _call_fwd(lib, d, c):
    a = d.a
    with torch.cuda.device(DEV):
        return lib.gae_decoder_dense(d.ptr("Z"), d.ptr("mask") if c["mask"] else None, a.ld("Z"), c["n"], c["d"],
                                     d.ptr("out"), a.ld("out"), _stream())


@pytest.mark.parametrize("c", L.FWD, ids=[c["id"] for c in L.FWD])
def test_decoder_dense(c):
    lib = _lib()
    arena, Z, mask = _fwd_arena(c)
    d = Device(arena)
    rc = _call_fwd(lib, d, c)
    kind = _kind()
    d.download()
    assert rc == 0, (c["id"], rc, lib.gae_last_error())
    assert kind == c["kind"], (c["id"], kind)
    d.check_memory(c["id"], ["Z"] + (["mask"] if c["mask"] else []), ["out"])
    ref, bound = L.decoder_dense(Z, mask)
    got = arena.get("out")
    _within(f"{c['id']} [{kind}: {L.fwd_kind(c)[1]}]", "out", got, ref, bound)
    sym = np.array_equal(got.view(np.uint32), got.T.view(np.uint32))
    print(f"{c['id']}: out {'is' if sym else 'is NOT'} bit-symmetric")      # recorded, not asserted: nothing documents it
    # a second identical call: the same bits
    first = arena.bits("out")
    assert _call_fwd(lib, d, c) == 0
    d.download()
    assert np.array_equal(arena.bits("out"), first), (c["id"], "second call differs")


# ---------------------------------------------------------------------------------------------- gae_decoder_dense_bwd
def _bwd_arena(c, with_mask, ws_bytes):
    n, d = c["n"], c["d"]
    Z, mask, G = L.decoder_inputs(n, d)
    ldz = R.lead(d, c["ld_Z"])
    a = R.Arena()
    a.add("G", n, n, L.ld_of(n, c["ld_G"]), c["mis_G"], G)
    a.add("Z", n, d, ldz, c["mis_Z"], Z)
    if with_mask:
        a.add("mask", n, d, ldz, c["mis_m"], mask)
    a.add("dZ", n, d, R.lead(d, c["ld_dZ"]), c["mis_dZ"])
    a.add_workspace("ws", ws_bytes)
    return a.build(), G, Z, (mask if with_mask else None)


def _call_bwd(lib, d, n, dd, with_mask, ws_bytes, ldg=None, ldz=None, lddz=None):
    a = d.a
    with torch.cuda.device(DEV):
        return lib.gae_decoder_dense_bwd(d.ptr("G"), a.ld("G") if ldg is None else ldg, d.ptr("Z"),
                                         d.ptr("mask") if with_mask else None, a.ld("Z") if ldz is None else ldz, n, dd,
                                         d.ptr("dZ"), a.ld("dZ") if lddz is None else lddz, d.ptr("ws"), ws_bytes, _stream())


@pytest.mark.parametrize("with_mask", [1, 0], ids=["mask", "nomask"])
@pytest.mark.parametrize("c", L.BWD, ids=[c["id"] for c in L.BWD])
def test_decoder_dense_bwd(c, with_mask, tuning):
    lib = _lib()
    n, dd = c["n"], c["d"]
    tuning("atb_bf16", c["atb_bf16"])
    ws_bytes = int(lib.gae_decoder_dense_bwd_workspace_bytes(n, dd))
    assert ws_bytes == L.bwd_workspace_bytes(n, dd, c["atb_bf16"])
    arena, G, Z, mask = _bwd_arena(c, with_mask, ws_bytes)
    d = Device(arena)
    rc = _call_bwd(lib, d, n, dd, with_mask, ws_bytes)
    kind = _kind()
    d.download()
    what = f"{c['id']}-{'mask' if with_mask else 'nomask'}"
    assert rc == 0, (what, rc, lib.gae_last_error())
    assert kind == c["kind"], (what, kind)
    d.check_memory(what, ["G", "Z"] + (["mask"] if with_mask else []), ["dZ"])
    slots, _, stride = R.atb_plan(n, dd, n, c["atb_bf16"])
    assert (arena.bits("ws").reshape(-1)[slots * stride:] == R.PATTERN).all(), (what, "workspace written behind the last slot")
    ref, bound = L.decoder_dense_bwd(G, Z, mask, c["atb_bf16"] if kind == "atb_bf16" else 0)
    _, inst, term1 = L.bwd_kind(c, with_mask)
    _within(f"{what} [{kind}: {inst}; term 1 {term1}; {slots} slots]", "dZ", arena.get("dZ"), ref, bound)
    # no atomics anywhere in the call: a second identical call gives the same bits
    first = arena.bits("dZ")
    assert _call_bwd(lib, d, n, dd, with_mask, ws_bytes) == 0
    d.download()
    assert np.array_equal(arena.bits("dZ"), first), (what, "second call differs")
    assert arena.guards_intact()


# ---------------------------------------------------------------------------------------------- gae_bce_logits
def _bce_arena(c, x, y, alias):
    rows, cols = c["rows"], c["cols"]
    a = R.Arena()
    a.add("x", rows, cols, R.lead(cols, c["ld_x"]), c["mis_x"], x)
    a.add("y", rows, cols, R.lead(cols, c["ld_y"]), c["mis_y"], y)
    if c["mode"] == "grad" or (c["mode"] == "alias" and not alias):
        a.add("g", rows, cols, R.lead(cols, c["ld_g"]), c["mis_g"])
    a.add("loss", 1, 1)
    a.add_workspace("ws", L.BCE_WORKSPACE_BYTES)
    return a.build()


def _call_bce(lib, d, c, grad):
    """grad: the name of the operand that takes the gradient, or None"""
    a = d.a
    with torch.cuda.device(DEV):
        return lib.gae_bce_logits(d.ptr("x"), a.ld("x"), d.ptr("y"), a.ld("y"), c["rows"], c["cols"], c["pw"],
                                  d.ptr("loss"), d.ptr(grad) if grad else None, a.ld(grad) if grad else 0, d.ptr("ws"),
                                  L.BCE_WORKSPACE_BYTES, _stream())


@pytest.mark.parametrize("c", L.BCE, ids=[c["id"] for c in L.BCE])
def test_bce_logits(c):
    lib = _lib()
    assert lib.gae_bce_logits_workspace_bytes() == L.BCE_WORKSPACE_BYTES
    x, y = L.bce_inputs(c)
    ref = L.bce_logits(x, y, c["pw"])
    # the call with a gradient buffer of its own (none for mode "null")
    arena = _bce_arena(c, x, y, alias=False)
    d = Device(arena)
    grad = None if c["mode"] == "null" else "g"
    rc = _call_bce(lib, d, c, grad)
    d.download()
    assert rc == 0, (c["id"], rc, lib.gae_last_error())
    d.check_memory(c["id"], ["x", "y"], ["loss"] + ([grad] if grad else []))
    loss = float(arena.get("loss")[0, 0])
    ratio = abs(loss - ref["loss"]) / ref["loss_bound"]
    print(f"{c['id']}: loss {loss!r}, fp64 {ref['loss']!r}, error / bound {ratio:.3f}")
    assert ratio <= 1.0, (c["id"], loss, ref["loss"], ref["loss_bound"])
    if grad:
        _within(c["id"], "grad", arena.get("g"), ref["grad"], ref["grad_bound"])
    # a second identical call: the same bits (ordered fp64 reduction)
    first_loss, first_g = arena.bits("loss"), (arena.bits("g") if grad else None)
    assert _call_bce(lib, d, c, grad) == 0
    d.download()
    assert np.array_equal(arena.bits("loss"), first_loss) and (not grad or np.array_equal(arena.bits("g"), first_g))
    if c["mode"] != "alias":
        return
    # grad == logits: the gradient lands over the logits, bit for bit the separate buffer's; labels and pads untouched
    arena2 = _bce_arena(c, x, y, alias=True)
    d2 = Device(arena2)
    rc = _call_bce(lib, d2, c, "x")
    d2.download()
    assert rc == 0, (c["id"], rc, lib.gae_last_error())
    d2.check_memory(c["id"] + " aliased", ["y"], ["loss", "x"])
    assert np.array_equal(arena2.bits("x"), first_g), (c["id"], "aliased gradient differs from the separate one",
                                                       int((arena2.bits("x") != first_g).sum()))
    assert np.array_equal(arena2.bits("loss"), first_loss)


# ---------------------------------------------------------------------------------------------- gae_csr_to_dense
@pytest.mark.parametrize("c", L.CSR, ids=[c["id"] for c in L.CSR])
def test_csr_to_dense(c):
    lib = _lib()
    a = R.Arena().add("out", c["n_rows"], c["n_cols"], c["ld"], 0).build()
    d = Device(a)
    indptr = torch.from_numpy(c["indptr"]).to(DEV)
    indices = torch.from_numpy(np.concatenate([c["indices"], np.full(4, -1, np.int32)])).to(DEV)   # never NULL; -1 behind the end
    with torch.cuda.device(DEV):
        rc = lib.gae_csr_to_dense(indptr.data_ptr(), indices.data_ptr(), c["n_rows"], c["n_cols"], d.ptr("out"), c["ld"],
                                  _stream())
    d.download()
    assert rc == 0, (c["id"], rc, lib.gae_last_error())
    d.check_memory(c["id"], [], ["out"])
    assert np.array_equal(indptr.cpu().numpy(), c["indptr"]) and np.array_equal(indices.cpu().numpy()[:-4], c["indices"])
    ref = L.csr_to_dense(c["indptr"], c["indices"], c["n_rows"], c["n_cols"])
    got = a.get("out")
    assert np.array_equal(got, ref.astype(np.float32)), (c["id"], np.argwhere(got != ref)[:4].tolist())
    print(f"{c['id']}: {c['indices'].size} entries, largest count {int(ref.max()) if ref.size else 0}")


# ---------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_return_before_any_launch():
    lib = _lib()
    fwd = [c for c in L.FWD if (c["n"], c["d"], c["mask"]) == (129, 39, 1)][0]
    arena, _, _ = _fwd_arena(fwd)
    d = Device(arena)

    def dec(ldz=40, ldo=arena.ld("out"), n=129, dd=39):
        with torch.cuda.device(DEV):
            return lib.gae_decoder_dense(d.ptr("Z"), d.ptr("mask"), ldz, n, dd, d.ptr("out"), ldo, _stream())
    for what, rc in (("ldz < d", dec(ldz=38)), ("ldo < n", dec(ldo=128)), ("negative n", dec(n=-1))):
        assert rc == E_SIZE and lib.gae_last_error(), (what, rc)
    assert dec(n=0) == 0
    d.download()
    assert d.untouched()

    c = [c for c in L.BWD if (c["n"], c["d"], c["ld_G"]) == (129, 7, 132)][0]
    n, dd = c["n"], c["d"]
    ws_bytes = int(lib.gae_decoder_dense_bwd_workspace_bytes(n, dd))
    arena, *_ = _bwd_arena(c, 1, ws_bytes)
    d = Device(arena)
    for what, rc, code in (("ldg < n", _call_bwd(lib, d, n, dd, 1, ws_bytes, ldg=n - 1), E_SIZE),
                           ("ldz < d", _call_bwd(lib, d, n, dd, 1, ws_bytes, ldz=dd - 1), E_SIZE),
                           ("lddz < d", _call_bwd(lib, d, n, dd, 1, ws_bytes, lddz=dd - 1), E_SIZE),
                           ("workspace one byte short", _call_bwd(lib, d, n, dd, 1, ws_bytes - 1), E_WORKSPACE),
                           ("no workspace", _call_bwd(lib, d, n, dd, 1, 0), E_WORKSPACE)):
        assert rc == code and lib.gae_last_error(), (what, rc)
    assert _call_bwd(lib, d, 0, dd, 1, ws_bytes) == 0 and _call_bwd(lib, d, n, 0, 1, ws_bytes) == 0
    d.download()
    assert d.untouched()

    bce = [c for c in L.BCE if (c["rows"], c["mode"], c["pw"]) == (16, "grad", 1023.0)][0]
    arena = _bce_arena(bce, *L.bce_inputs(bce), alias=False)
    d = Device(arena)

    def loss_call(ldx=arena.ld("x"), ldy=arena.ld("y"), ldg=arena.ld("g"), loss=True, nbytes=L.BCE_WORKSPACE_BYTES, rows=16,
                  cols=16):
        with torch.cuda.device(DEV):
            return lib.gae_bce_logits(d.ptr("x"), ldx, d.ptr("y"), ldy, rows, cols, 37.5, d.ptr("loss") if loss else None,
                                      d.ptr("g"), ldg, d.ptr("ws"), nbytes, _stream())
    for what, rc, code in (("ldx < cols", loss_call(ldx=15), E_SIZE), ("ldy < cols", loss_call(ldy=15), E_SIZE),
                           ("ldg < cols", loss_call(ldg=15), E_SIZE), ("loss_out NULL", loss_call(loss=False), E_NULL),
                           ("workspace one byte short", loss_call(nbytes=L.BCE_WORKSPACE_BYTES - 1), E_WORKSPACE),
                           ("negative rows", loss_call(rows=-1), E_SIZE)):
        assert rc == code and lib.gae_last_error(), (what, rc)
    d.download()
    assert d.untouched()
    # an empty matrix: nothing but loss = 0 is written
    for rows, cols in ((0, 16), (16, 0)):
        assert loss_call(rows=rows, cols=cols, ldx=max(cols, 1), ldy=max(cols, 1), ldg=max(cols, 1)) == 0
        d.download()
        assert arena.bits("loss").tolist() == [[0]] and arena.guards_intact()
        assert (arena.bits("g") == R.PATTERN).all() and (arena.bits("ws") == R.PATTERN).all()
        d.dev[arena.offset("loss")] = R.PATTERN

    csr = L.CSR[0]
    a = R.Arena().add("out", csr["n_rows"], csr["n_cols"], csr["ld"], 0).build()
    d = Device(a)
    indptr, indices = torch.from_numpy(csr["indptr"]).to(DEV), torch.from_numpy(csr["indices"]).to(DEV)
    with torch.cuda.device(DEV):
        rc = lib.gae_csr_to_dense(indptr.data_ptr(), indices.data_ptr(), csr["n_rows"], csr["n_cols"], d.ptr("out"),
                                  csr["n_cols"] - 1, _stream())
    assert rc == E_SIZE
    d.download()
    assert d.untouched()


# ---------------------------------------------------------------------------------------------- the Python wrappers
@pytest.mark.parametrize("n,d,entry", L.CHAIN, ids=["n%d-d%d-%s" % c for c in L.CHAIN])
def test_chain_through_the_wrappers(n, d, entry):
    """ops.bce_with_logits(ops.decoder_dense(Z, mask), ops.csr_to_dense(...), pw) and ops.backward -- the inductive
    trainer's loss -- and ops.decoder_bce above FUSED_MAX_D, on graphs with duplicate edges: per element
    |dZ - ref| <= 5e-5 max|ref| with NO floor under max|ref| (the convention of test_gpu_loss_range.py; a mean-loss
    gradient is far below 1, so a floor of 1 would make the bound absolute)"""
    import gae_dgl_amd as G
    from gae_dgl_amd import ops
    Z, mask, src, dst = L.chain_inputs(n, d)
    ref_loss, ref_dZ, pw, A = L.chain_ref(Z, mask, src, dst)
    gr = G.DGLGraph((src, dst), num_nodes=n).to(torch.device(DEV))
    Zd = torch.from_numpy(Z).to(DEV).requires_grad_(True)
    md = torch.from_numpy(mask).to(DEV)
    if entry == "dense":
        indptr, indices = gr.csr()
        label = ops.csr_to_dense(indptr, indices, n, n)
        assert np.array_equal(label.cpu().numpy(), A.astype(np.float32))
        loss = ops.bce_with_logits(ops.decoder_dense(Zd, md), label, pw)
    else:
        assert d > ops.FUSED_MAX_D
        loss = ops.decoder_bce(Zd, md, gr)
    ops.backward(loss)
    kind = _kind()
    loss = loss.detach()
    got = Zd.grad.cpu().numpy().astype(np.float64)
    top = float(np.abs(ref_dZ).max())
    err = float(np.abs(got - ref_dZ).max())
    print(f"chain n {n} d {d} {entry}: backward ends with {kind}; max|ref dZ| {top:.3e}, max|dZ - ref| / max|ref| "
          f"{err / top:.3e}; loss {float(loss)!r}, fp64 {ref_loss!r}")
    assert kind == {129: "atb_scalar", 132: "atb_bf16", 131: "atb_scalar"}[n], kind
    assert abs(float(loss) - ref_loss) <= 1e-5 * max(1.0, abs(ref_loss))
    assert top < 1.0 and err <= 5e-5 * top, (err, top)


def test_decoder_dense_raw_takes_a_column_slice_of_a_wider_tensor():
    """Z a column slice (row stride 24, 16 columns), the mask contiguous: the ABI has one ldz for both, so the wrapper
    must not hand the slice's stride to the mask -- the same bits as contiguous copies of both"""
    from gae_dgl_amd import ops
    n, d = 129, 16
    Z, mask, _ = L.decoder_inputs(n, d)
    wide = torch.full((n, d + 8), float("nan"), device=DEV)
    wide[:, 3:3 + d] = torch.from_numpy(Z).to(DEV)
    Zs, md = wide[:, 3:3 + d], torch.from_numpy(mask).to(DEV)
    assert Zs.stride(0) == d + 8 and not Zs.is_contiguous()
    for m in (md, None):
        got, want = ops.decoder_dense_raw(Zs, m), ops.decoder_dense_raw(Zs.contiguous(), m)
        assert torch.equal(got, want) and bool(torch.isfinite(got).all())
        ref, bound = L.decoder_dense(Z, None if m is None else mask)
        _within("column slice" + (" with mask" if m is not None else ""), "out", got.cpu().numpy(), ref, bound)
    one = ops.decoder_dense_raw(Zs[:1], md[:1])          # a single row has no stride to compare
    assert torch.equal(one, ops.decoder_dense_raw(Zs[:1].contiguous(), md[:1]))
