"""gae_linear_fwd / gae_linear_bwd / gae_x_linear_bwd_partials (K3-K5, csrc/dense.hip) through the raw C ABI against
tests/dense_ref.py.  Every case places its operands in one arena (NaN guards of 64 floats around each operand, NaN pad
columns [width, ld), a base 0 or 1 float past a 16-byte boundary, a workspace of exactly the queried size), makes ONE
call and asserts: status 0 and dense_last_kind == the kernel the case was built for; every output element within its
derived rounding bound of float64 (dense_ref.linear_fwd / linear_bwd; no bound was widened, see MEASUREMENTS.md
"Dense layer kernels in guarded arenas"); guards intact; inputs bit-unchanged, pads included; output pad columns
still the pattern; no NaN in an output.

dense_last_kind -> cases (ids of dense_ref.FWD / dense_ref.BWD; test_dense_ref_cpu.py asserts the restated dispatch
sends each case there and prints the template instances):
  1 rows          FWD rows-* (gemm_rows = 2, f_in 1 .. 64); BWD dM-*-rows (dM with f_out <= 64)
  2 pieces        FWD pieces-* (f_in 128, 129, 130, 192 and 2049 without a workspace; W aligned and not)
  3 wlds          FWD wlds-default-* (f_in 2049, split-K), wlds-forced-* (linear_wlds = 2; f_in 32, 39, 64, 520)
  4 stream        FWD stream-* (gemm_rows = 0 on the short rows; unaligned or unsplit long rows; f_out 33, 65);
                  BWD dM-* (f_in <= 128)
  5 stream+split  FWD split-* (f_in 520 and, with linear_wlds = 0, 2049; W aligned and not)
  6 tiled         FWD tiled-* (f_out 130); BWD dM-*-tiled (f_in 130)
  7 xw            FWD xw-* (f_in 200 and 2049, rows of whole vectors)
  8 atb_bf16      BWD bf16-* (atb_bf16 = 1), bf16=2-*
  9 atb_narrow    BWD narrow-* (f_in <= 32, and db alone)
 10 atb_vec       BWD vec-* (atb_bf16 = 0, or f_out > 32)
 11 atb_scalar    BWD scalar-* (rows of M that are not whole vectors)
A gae_linear_bwd call that wants dM ends with dM's kernel: its weight-gradient kernel is pinned by the same shape in
test_partials_are_the_first_half_of_linear_bwd or by a case without dM."""
import ctypes

import numpy as np
import pytest
import torch

import adam_ref
import dense_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E_NULL, E_SIZE, E_ALIGN, E_DTYPE, E_WORKSPACE = -1, -2, -3, -4, -5


class Device:
    """a dense_ref.Arena and its copy on the GPU"""

    def __init__(self, arena):
        self.a = arena
        self.dev = torch.from_numpy(arena.host.view(np.int32).copy()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.before = arena.host.copy()

    def ptr(self, name, offset_floats=0):
        return self.dev.data_ptr() + 4 * (self.a.offset(name) + offset_floats)

    def download(self):
        torch.cuda.synchronize()
        self.a.host = self.dev.cpu().numpy().view(np.uint32).copy()

    def untouched(self):
        return np.array_equal(self.a.host, self.before)

    def check_memory(self, what, inputs, outputs):
        """guards intact, inputs bit-unchanged with their pads, output pads still the pattern, no NaN in an output"""
        a = self.a
        assert a.guards_intact() and all(a.pads_intact(k) for k in a.ops), \
            (what, "written outside an operand (word, nearest operand, offset from its base):", a.damaged())
        for name in inputs:
            o = a.ops[name]
            assert np.array_equal(a.footprint(name), self.before[o["base"]:o["base"] + o["rows"] * o["ld"]]), \
                (what, f"input {name} changed")
        for name in outputs:
            assert a.pads_intact(name), (what, f"pad columns of {name} written")
            got = a.get(name)
            assert not np.isnan(got).any(), (what, f"NaN in {name}", np.argwhere(np.isnan(got))[:4].tolist())


def _stream():
    from gae_dgl_amd.ops import _stream as s
    return s()


def _kind():
    from gae_dgl_amd import _lib
    return R.KIND_NAMES.get(_lib.tuning_get("dense_last_kind"), "none")


def _within(what, name, got, ref, bound, kblock=None):
    ratio, where = R.worst_element(got, ref, bound, kblock=kblock)
    print(f"{what}: {name} largest error / bound {ratio:.3f} ({where})")
    assert ratio <= 1.0, (what, name, ratio, where)


# ---------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("c", R.FWD, ids=[c["id"] for c in R.FWD])
def test_linear_fwd(c, tuning):
    from gae_dgl_amd import _lib
    lib = _lib.load()
    n, K, J = c["n"], c["f_in"], c["f_out"]
    tuning("gemm_rows", c["gemm_rows"]); tuning("linear_wlds", c["linear_wlds"])
    M, W, b = R.draw(11, n, K), R.draw(12, J, K), (R.draw(13, J) if c["bias"] else None)
    a = R.Arena()
    a.add("M", n, K, R.lead(K, c["ld_M"]), c["mis_M"], M)
    a.add("W", J, K, None, c["mis_W"], W)
    if b is not None:
        a.add("b", 1, J, None, c["mis_b"], b)
    a.add("Y", n, J, R.lead(J, c["ld_Y"]), c["mis_Y"])
    ws_bytes = int(lib.gae_linear_fwd_workspace_bytes(n, K, J)) if c["ws"] else 0
    if c["ws"]:
        assert ws_bytes > 0
        a.add_workspace("ws", ws_bytes)
    d = Device(a.build())
    with torch.cuda.device(DEV):
        rc = lib.gae_linear_fwd(d.ptr("M"), a.ld("M"), n, K, d.ptr("W"), d.ptr("b") if b is not None else None, J, c["act"],
                                d.ptr("Y"), a.ld("Y"), d.ptr("ws") if c["ws"] else None, ws_bytes, _stream())
    kind = _kind()
    d.download()
    assert rc == 0, (c["id"], rc, lib.gae_last_error())
    assert kind == c["kind"], (c["id"], kind)
    d.check_memory(c["id"], ["M", "W"] + (["b"] if b is not None else []), ["Y"])
    ref, bound = R.linear_fwd(M, W, b, c["act"])
    _within(c["id"], "Y", d.a.get("Y"), ref, bound)


# ---------------------------------------------------------------------------------------------- backward
def _bwd_arena(n, f_in, f_out, act, ld_dY="w", mis_dY=0, ld_Y="w", mis_Y=0, ld_M="w", mis_M=0, mis_W=0, ld_dM="w",
               mis_dM=0, ws_bytes=0, seed=0):
    dY, Y = R.draw(21 + seed, n, f_out), R.draw_mask(22 + seed, n, f_out)
    M, W = R.draw(23 + seed, n, f_in), R.draw(24 + seed, f_out, f_in)
    a = R.Arena()
    a.add("dY", n, f_out, R.lead(f_out, ld_dY), mis_dY, dY)
    if act == R.ACT_RELU:
        a.add("Y", n, f_out, R.lead(f_out, ld_Y), mis_Y, Y)
    a.add("M", n, f_in, R.lead(f_in, ld_M), mis_M, M)
    a.add("W", f_out, f_in, None, mis_W, W)
    a.add("dW", f_out, f_in)
    a.add("db", 1, f_out)
    a.add("dM", n, f_in, R.lead(f_in, ld_dM), mis_dM)
    a.add_workspace("ws", ws_bytes)
    return a.build(), (dY, Y, M, W)


def _call_bwd(lib, d, n, f_in, f_out, act, want, ws_bytes):
    a = d.a
    relu = act == R.ACT_RELU
    with torch.cuda.device(DEV):
        return lib.gae_linear_bwd(d.ptr("dY"), a.ld("dY"), d.ptr("Y") if relu else None, a.ld("Y") if relu else 0, act,
                                  d.ptr("M"), a.ld("M"), d.ptr("W"), n, f_in, f_out,
                                  d.ptr("dW") if "dW" in want else None, d.ptr("db") if "db" in want else None,
                                  d.ptr("dM") if "dM" in want else None, a.ld("dM"), d.ptr("ws"), ws_bytes, _stream())


@pytest.mark.parametrize("c", R.BWD, ids=[c["id"] for c in R.BWD])
def test_linear_bwd(c, tuning):
    from gae_dgl_amd import _lib
    lib = _lib.load()
    n, f_in, f_out, act, want = c["n"], c["f_in"], c["f_out"], c["act"], c["want"]
    tuning("gemm_rows", c["gemm_rows"]); tuning("atb_bf16", c["atb_bf16"])
    ws_bytes = int(lib.gae_linear_bwd_workspace_bytes(n, f_in, f_out))
    assert ws_bytes == R.bwd_workspace_bytes(n, f_in, f_out, c["atb_bf16"])
    arena, (dY, Y, M, W) = _bwd_arena(n, f_in, f_out, act, c["ld_dY"], c["mis_dY"], c["ld_Y"], c["mis_Y"], c["ld_M"],
                                      c["mis_M"], c["mis_W"], c["ld_dM"], c["mis_dM"], ws_bytes)
    d = Device(arena)
    rc = _call_bwd(lib, d, n, f_in, f_out, act, want, ws_bytes)
    kind = _kind()
    d.download()
    assert rc == 0, (c["id"], rc, lib.gae_last_error())
    assert kind == c["kind"], (c["id"], kind)
    d.check_memory(c["id"], ["dY", "M", "W"] + (["Y"] if act == R.ACT_RELU else []), list(want))
    for name in ("dW", "db", "dM"):
        if name not in want:        # an output that was not asked for is not written
            assert (arena.bits(name) == R.PATTERN).all(), (c["id"], f"{name} written though NULL was passed")
    # the weight-gradient kernel in use decides dW's bound: exact fp32 products unless atb_bf16_kernel ran
    form = c["atb_bf16"] if R.wgrad_kind(c)[0] == "atb_bf16" else 0
    refs = R.linear_bwd(dY, Y, act, M, W, form)
    for name in want:
        ref, bound = refs[name]
        _within(c["id"], name, arena.get(name).reshape(ref.shape), ref, bound, kblock=8 if name == "dW" else None)


# ---------------------------------------------------------------------------------------------- the partial lists
@pytest.mark.parametrize("p", R.PARTIALS, ids=lambda p: "n%d-i%d-o%d-dW%d-db%d-act%d-bf16=%d-M%d%s" % p)
def test_partials_are_the_first_half_of_linear_bwd(p, tuning):
    """layout triple == the restated plan; the slots added on the host in fp32 in the library's order for a flat list
    (adam_ref.sum_in_library_order) == gae_linear_bwd's dW / db bit for bit; nothing behind the last slot is written"""
    from gae_dgl_amd import _lib
    lib = _lib.load()
    n, f_in, f_out, want_dW, want_db, act, bf16, mis_M, ld_M = p
    tuning("atb_bf16", bf16)
    ws_bytes = int(lib.gae_linear_bwd_workspace_bytes(n, f_in, f_out))
    slots, _, stride = R.atb_plan(n, f_out, f_in, bf16)
    assert ws_bytes == R.bwd_workspace_bytes(n, f_in, f_out, bf16) and slots * stride * 4 <= ws_bytes - 256
    arena, _ = _bwd_arena(n, f_in, f_out, act, ld_M=ld_M, mis_M=mis_M, ws_bytes=ws_bytes, seed=100)
    d = Device(arena)
    relu = act == R.ACT_RELU
    lay = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    with torch.cuda.device(DEV):
        rc = lib.gae_x_linear_bwd_partials(d.ptr("dY"), arena.ld("dY"), d.ptr("Y") if relu else None,
                                           arena.ld("Y") if relu else 0, act, d.ptr("M"), arena.ld("M"), n, f_in, f_out,
                                           want_dW, want_db, d.ptr("ws"), ws_bytes, lay, _stream())
    kind = _kind()
    d.download()
    assert rc == 0, (rc, lib.gae_last_error())
    I = f_in if want_dW else 0
    assert list(lay)[:3] == [slots, stride, f_out * I] and lay[3] == -1, list(lay)
    want_kind = R.atb_kind(f_out, I, arena.ld("M") if want_dW else arena.ld("dY"), not mis_M if want_dW else True, bf16)[0]
    assert kind == want_kind, (kind, want_kind)
    d.check_memory(str(p), ["dY", "M", "W"] + (["Y"] if relu else []), [])
    assert all((arena.bits(k) == R.PATTERN).all() for k in ("dW", "db", "dM"))
    ws = arena.bits("ws").reshape(-1)
    assert (ws[slots * stride:] == R.PATTERN).all(), "workspace written behind the last slot"
    lists = {}
    for q in range(slots):          # inside a slot: the [f_out, I] tile, then f_out column sums, then nothing
        used = f_out * I + (f_out if want_db else 0)
        assert not np.isnan(ws[q * stride:q * stride + used].view(np.float32)).any(), q
        assert (ws[q * stride + f_out * I + (f_out if want_db else 0):(q + 1) * stride] == R.PATTERN).all(), q
    if want_dW:
        lists["dW"] = np.stack([ws[q * stride:q * stride + f_out * I] for q in range(slots)]).view(np.float32)
    if want_db:
        lists["db"] = np.stack([ws[q * stride + lay[2]:q * stride + lay[2] + f_out] for q in range(slots)]).view(np.float32)
    # the same call through gae_linear_bwd, in a fresh copy of the arena
    arena2, _ = _bwd_arena(n, f_in, f_out, act, ld_M=ld_M, mis_M=mis_M, ws_bytes=ws_bytes, seed=100)
    d2 = Device(arena2)
    assert _call_bwd(lib, d2, n, f_in, f_out, act, list(lists), ws_bytes) == 0
    d2.download()
    assert arena2.guards_intact()
    for name, P in lists.items():
        got = arena2.get(name).reshape(-1)
        want = adam_ref.sum_in_library_order(P)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            (name, slots, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    print(f"{p}: {slots} slots of {stride} floats, {kind}")


# ---------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_return_before_any_launch():
    from gae_dgl_amd import _lib
    lib = _lib.load()
    n, f_in, f_out = 33, 39, 16
    fwd_ws = 4096
    a = R.Arena()
    a.add("M", n, f_in, 40, 0, R.draw(1, n, f_in)).add("W", f_out, f_in, None, 0, R.draw(2, f_out, f_in))
    a.add("b", 1, f_out, None, 0, R.draw(3, f_out)).add("Y", n, f_out, 20, 0).add_workspace("ws", fwd_ws + 16)
    d = Device(a.build())
    s = _stream()

    def fwd(ldm=40, n_=n, f_out_=f_out, act=R.ACT_RELU, ldy=20, ws_off=0):
        with torch.cuda.device(DEV):
            return lib.gae_linear_fwd(d.ptr("M"), ldm, n_, f_in, d.ptr("W"), d.ptr("b"), f_out_, act, d.ptr("Y"), ldy,
                                      d.ptr("ws", ws_off), fwd_ws, s)
    for what, rc, code in (("ldm < f_in", fwd(ldm=f_in - 1), E_SIZE), ("ldy < f_out", fwd(ldy=f_out - 1), E_SIZE),
                           ("bad act", fwd(act=2), E_DTYPE), ("negative n", fwd(n_=-1), E_SIZE),
                           ("misaligned workspace", fwd(ws_off=1), E_ALIGN)):
        assert rc == code and lib.gae_last_error(), (what, rc)
    assert fwd(n_=0) == 0 and fwd(f_out_=0, ldy=0) == 0
    d.download()
    assert d.untouched()

    ws_bytes = int(lib.gae_linear_bwd_workspace_bytes(n, f_in, f_out))
    arena, _ = _bwd_arena(n, f_in, f_out, R.ACT_RELU, ld_dY="4", ld_Y="4", ld_M="4", ld_dM="4", ws_bytes=ws_bytes + 16)
    d = Device(arena)

    def bwd(lddy=20, ldy=20, ldm=40, act=R.ACT_RELU, Y=True, n_=n, f_out_=f_out, ws_off=0, nbytes=ws_bytes, dM=True):
        with torch.cuda.device(DEV):
            return lib.gae_linear_bwd(d.ptr("dY"), lddy, d.ptr("Y") if Y else None, ldy, act, d.ptr("M"), ldm, d.ptr("W"),
                                      n_, f_in, f_out_, d.ptr("dW"), d.ptr("db"), d.ptr("dM") if dM else None, 40,
                                      d.ptr("ws", ws_off), nbytes, s)
    for what, rc, code in (("lddy < f_out", bwd(lddy=f_out - 1), E_SIZE), ("RELU without Y", bwd(Y=False), E_NULL),
                           ("ldy < f_out", bwd(ldy=f_out - 1), None), ("ldm < f_in", bwd(ldm=f_in - 1), None),
                           ("bad act", bwd(act=-1), E_DTYPE), ("workspace one byte short", bwd(nbytes=ws_bytes - 1), E_WORKSPACE),
                           ("no workspace", bwd(nbytes=0), E_WORKSPACE), ("misaligned workspace", bwd(ws_off=1), E_ALIGN)):
        assert (rc == code if code is not None else rc < 0) and lib.gae_last_error(), (what, rc)
    d.download()
    assert d.untouched()
    # empty calls: f_out == 0 writes nothing; n == 0 writes nothing to dM [0, f_in] and the empty sums dW = db = 0
    assert bwd(f_out_=0, lddy=0, ldy=0) == 0
    d.download()
    assert d.untouched()
    assert bwd(n_=0) == 0
    d.download()
    assert arena.guards_intact() and all(arena.pads_intact(k) for k in arena.ops)
    assert all(np.array_equal(arena.footprint(k), d.before[arena.offset(k):arena.offset(k) + arena.footprint(k).size])
               for k in ("dY", "Y", "M", "W", "dM"))
    assert not arena.bits("dW").any() and not arena.bits("db").any()
