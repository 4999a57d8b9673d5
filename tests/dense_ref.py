"""Reference for K3-K5 (gae_linear_fwd / gae_linear_bwd / gae_x_linear_bwd_partials, csrc/dense.hip), numpy only: an
arena that places every operand of one call between NaN guards, the float64 results, a rounding bound per output
element, a host restatement of which kernel a call takes (written from the conditions of dispatch_gemm /
launch_gemm_stream / launch_atb / gae_linear_fwd; used to pick cases and to label failures, never to excuse one), and
the case tables that tests/test_dense_ref_cpu.py and tests/test_gpu_dense_abi.py share."""
import numpy as np

GUARD = 64                 # floats in front of and behind every operand
PATTERN = 0x7FC0BEEF       # a quiet NaN: guards, pad columns [width, ld), outputs and workspace before the call
U24 = 2.0 ** -24           # unit roundoff of fp32
ACT_IDENTITY, ACT_RELU = 0, 1

# dense_last_kind (include/gae_hip.h)
KINDS = {"rows": 1, "pieces": 2, "wlds": 3, "stream": 4, "stream+split": 5, "tiled": 6, "xw": 7, "atb_bf16": 8,
         "atb_narrow": 9, "atb_vec": 10, "atb_scalar": 11}
KIND_NAMES = {v: k for k, v in KINDS.items()}


# ------------------------------------------------------------------ the arena
def lead(width, kind):
    """a leading dimension for rows of `width` floats: "w" the width itself, "4" the next multiple of 4 above the
    width's own (so that pad columns exist), "odd" an odd value above the width"""
    if kind == "w":
        return max(width, 1)
    if kind == "4":
        r = (width + 3) // 4 * 4
        return r if r > width else width + 4
    if kind == "odd":
        return width + 1 if width % 2 == 0 else width + 2
    raise ValueError(kind)


class Arena:
    """the operands of ONE call in one buffer of 32-bit words.  Every operand [rows, width] with leading dimension ld
    owns rows * ld words between two guards of GUARD words; its base is `misalign` floats (0 or 1) past a 16-byte
    boundary of the buffer (the buffer itself must start on one).  Guards and pad columns hold PATTERN; so do operands
    that were given no values (outputs) and the workspace.  `inside` marks the words that are elements of an operand
    or of the workspace."""

    def __init__(self):
        self.ops, self.pos, self.host = {}, 0, None

    def add(self, name, rows, width, ld=None, misalign=0, values=None):
        assert self.host is None and name not in self.ops and misalign in (0, 1)
        ld = max(width, 1) if ld is None else ld
        assert ld >= width and rows >= 0
        base = self.pos + GUARD
        base += (misalign - base) % 4
        span = max(rows * ld, 1)          # an empty operand owns one dummy word (never NULL); it counts as guard
        self.ops[name] = dict(base=base, rows=rows, width=width, ld=ld, values=values)
        self.pos = base + span + GUARD
        return self

    def add_workspace(self, name, nbytes):
        """16-byte aligned, exactly nbytes long (rounded up to whole words)"""
        return self.add(name, 1, (nbytes + 3) // 4, None, 0, None)

    def build(self):
        self.host = np.full(self.pos, PATTERN, np.uint32)
        self.inside = np.zeros(self.pos, bool)
        self.pad = {}
        for name, o in self.ops.items():
            idx = self.index(name)
            self.inside[idx] = True
            if o["values"] is not None:
                v = np.ascontiguousarray(o["values"], np.float32).reshape(o["rows"], o["width"])
                self.host[idx] = v.view(np.uint32)
            full = o["base"] + np.arange(o["rows"] * o["ld"], dtype=np.int64).reshape(o["rows"], o["ld"])
            self.pad[name] = full[:, o["width"]:].reshape(-1)
        assert not self.inside[np.concatenate([p for p in self.pad.values()] + [np.zeros(0, np.int64)])].any()
        return self

    def index(self, name):
        o = self.ops[name]
        r = np.arange(o["rows"], dtype=np.int64)[:, None]
        return o["base"] + r * o["ld"] + np.arange(o["width"], dtype=np.int64)[None, :]

    def offset(self, name):
        """float offset of the operand's first element in the buffer"""
        return self.ops[name]["base"]

    def ld(self, name):
        return self.ops[name]["ld"]

    def bits(self, name):
        return self.host[self.index(name)].copy()

    def get(self, name):
        return self.bits(name).view(np.float32)

    def footprint(self, name):
        """all rows * ld words of the operand, pads included"""
        o = self.ops[name]
        return self.host[o["base"]:o["base"] + o["rows"] * o["ld"]].copy()

    def guards_intact(self):
        """every word that is neither an element nor a pad column still holds PATTERN"""
        free = ~self.inside
        for p in self.pad.values():
            free[p] = False
        return bool(np.all(self.host[free] == PATTERN))

    def pads_intact(self, name):
        return bool(np.all(self.host[self.pad[name]] == PATTERN))

    def damaged(self):
        """offsets of the words outside every operand that no longer hold PATTERN, with the nearest operand"""
        bad = np.flatnonzero(~self.inside & (self.host != PATTERN))
        out = []
        for w in bad[:8]:
            name = min(self.ops, key=lambda k: min(abs(int(w) - self.ops[k]["base"]),
                                                   abs(int(w) - self.ops[k]["base"] - self.ops[k]["rows"] * self.ops[k]["ld"])))
            out.append((int(w), name, int(w) - self.ops[name]["base"]))
        return out


# ------------------------------------------------------------------ float64 references and bounds
def _f64(x):
    return np.asarray(x, np.float64)


def masked(dY, Y, act):
    """dYm = dY (.) [Y > 0] with the Y that is given (RELU), dY itself (identity)"""
    dY = _f64(dY)
    return np.where(_f64(Y) > 0.0, dY, 0.0) if act == ACT_RELU else dY


def linear_fwd(M, W, b, act):
    """(Y, bound): Y = act(M W^T + b) in float64; bound[i, j] = (K + 4) 2^-24 (sum_k |m_ik| |w_jk| + |b_j|) -- what ANY
    order of fp32 additions of the exact products stays within (the activation is 1-Lipschitz)"""
    M, W = _f64(M), _f64(W)
    K = M.shape[1]
    y = M @ W.T
    mag = np.abs(M) @ np.abs(W).T
    if b is not None:
        y = y + _f64(b)[None, :]
        mag = mag + np.abs(_f64(b))[None, :]
    if act == ACT_RELU:
        y = np.maximum(y, 0.0)
    return y, (K + 4) * U24 * mag


def linear_bwd(dY, Y, act, M, W, atb_bf16=1):
    """float64 (dW, db, dM) and their bounds.  dM: contraction length f_out.  dW / db: length n; with the bf16 forms
    of the weight-gradient kernel (atb_bf16 1: three pieces per operand, six pairs; 2: two pieces, three pairs) the
    bound of dW is that of wgrad_bound.  db is an fp32 sum in every form."""
    dYm = masked(dY, Y, act)
    n, f_out = dYm.shape
    out = {}
    if M is not None:
        M = _f64(M)
        out["dW"] = (dYm.T @ M, wgrad_bound(n, atb_bf16) * (np.abs(dYm).T @ np.abs(M)))
    out["db"] = (dYm.sum(0), (n + 4) * U24 * np.abs(dYm).sum(0))
    if W is not None:
        W = _f64(W)
        out["dM"] = (dYm @ W, (f_out + 4) * U24 * (np.abs(dYm) @ np.abs(W)))
    return out


def wgrad_bound(n, atb_bf16):
    """factor c of |dW_err| <= c sum_r |dYm_ro| |m_ri|:
    0 (exact fp32 products): (n + 4) 2^-24.
    1 (three bf16 pieces, 24 bits per operand, six pairs): the dropped pairs add a few 2^-24 per product, far below
      (n + 4) 2^-24 -- twice the fp32 bound.
    2 (two pieces: v = hi + lo + r with |r| <= 2^-16 |v|, bf16 keeps 8 significant bits per piece; pairs hi.hi, hi.lo,
      lo.hi): per product |r_a b| + |a r_b| + |lo_a lo_b| <= 3 2^-16 (1 + 2^-8) |a b| < 4 2^-16 |a b|, on top of the
      additions' 2 (n + 4) 2^-24."""
    base = (n + 4) * U24
    if atb_bf16 == 0:
        return base
    if atb_bf16 == 1:
        return 2 * base
    return 2 * base + 4 * 2.0 ** -16


def worst_element(got, ref, bound, tile_rows=32, tile_cols=32, kblock=None):
    """(ratio, text): the largest |got - ref| / bound and where it sits.  bound == 0 admits only got == ref."""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0, "empty"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    ratio = np.where(np.isnan(got), np.inf, ratio)
    flat = int(np.argmax(ratio))
    r, c = np.unravel_index(flat, ratio.shape) if ratio.ndim == 2 else (0, flat)
    rows, cols = ratio.shape if ratio.ndim == 2 else (1, ratio.shape[0])
    where = [f"row {r} col {c} of {rows} x {cols}: got {float(got.reshape(rows, cols)[r, c])!r}, "
             f"fp64 {float(ref.reshape(rows, cols)[r, c])!r}, "
             f"bound {bound.reshape(rows, cols)[r, c]:.3g}"]
    if r >= (rows - 1) // tile_rows * tile_rows:
        where.append("last row tile")
    if c >= (cols - 1) // tile_cols * tile_cols:
        where.append("last column group")
    if kblock and c >= (cols - 1) // kblock * kblock:
        where.append("last k-block")
    return float(ratio.reshape(-1)[flat]), ", ".join(where)


# ------------------------------------------------------------------ which kernel a call takes
K_GEMM_ROWS_MIN_N = 1 << 18


def stream_splits(n, K):
    """gemm_stream_splits"""
    tiles, kblocks = (n + 31) // 32, (K + 7) // 8
    if tiles >= 384 or kblocks < 64:
        return 1
    sp = min((768 + tiles - 1) // tiles, kblocks // 16, 32)
    return max(sp, 1)


def fwd_workspace_bytes_split(n, K, J):
    """the split-K share of gae_linear_fwd_workspace_bytes"""
    sp = stream_splits(n, K) if J <= 128 else 1
    return (sp * n * J * 4 + 255) // 256 * 256 if sp > 1 else 0


def gemm_kind(n, K, J, bt, pro, lda, a_aligned, ldb, b_aligned, ldam=0, am_aligned=True, ws_floats=0, gemm_rows=1,
              linear_wlds=1):
    """(kind, template instance) of dispatch_gemm<BT, PRO_A, MASK_B = false> on out[n, J] = A[n, K] B: the forward
    (bt, A = M, B = W [J, K]) and dM (not bt, A = dY with its mask operand when pro, B = W [K, J])"""
    K4 = (K + 3) // 4 * 4
    if J > 128:
        vec = lda % 4 == 0 and a_aligned and (not pro or (ldam % 4 == 0 and am_aligned))
        return "tiled", f"gemm_kernel<4, vec_a={int(vec)}>"
    nt = 1 if J <= 32 else 2 if J <= 64 else 4
    avec = lda % 4 == 0 and a_aligned and K >= 1 and (not pro or (ldam % 4 == 0 and am_aligned))
    bvec = bt and ldb % 4 == 0 and b_aligned and K >= 4 and K % 4 == 0
    if gemm_rows and nt <= 2 and 1 <= K <= 64 and n >= (1 if gemm_rows > 1 else K_GEMM_ROWS_MIN_N):
        av = avec and lda >= K4 and (not pro or ldam >= K4)
        return "rows", f"gemm_rows_kernel<{nt}, kb={4 if K <= 32 else 8}, avec={int(av)}>"
    splits = stream_splits(n, K) if ws_floats > 0 else 1
    if splits > 1 and ws_floats < splits * n * J:
        splits = 1
    kbps = ((K + 7) // 8 + splits - 1) // splits
    if nt == 1 and bt and not pro and K >= 128 and avec and lda >= K4 and n > 0:
        wvec = ldb % 4 == 0 and b_aligned and ldb >= K4
        return "pieces", f"linear_fwd_pieces_kernel<wvec={int(wvec)}> splits={splits}"
    if nt == 1 and bt and not pro and kbps <= 64 and n > 0 and \
            (K >= 32 if linear_wlds > 1 else (linear_wlds == 1 and splits > 1 and K >= 2048)):
        wvec = ldb % 4 == 0 and b_aligned
        return "wlds", f"linear_fwd_wlds_kernel<avec={int(avec)}, wvec={int(wvec)}> splits={splits}"
    return ("stream+split" if splits > 1 else "stream"), \
        f"gemm_stream_kernel<{nt}, avec={int(avec)}, bvec={int(bvec)}> splits={splits}"


def xw_usable(aligned, ldx, n, K, J):
    """gae::xw_usable for fp32 rows"""
    return n > 0 and 193 <= K < (1 << 24) and 1 <= J <= 32 and (ldx * 4) % 16 == 0 and ldx >= K and aligned and \
        n * ldx * 4 < 0xE0000000


def fwd_kind(n, K, J, ldm, m_aligned, w_aligned, ws_bytes=0, xw_ws_bytes=0, gemm_rows=1, linear_wlds=1):
    """gae_linear_fwd.  xw_ws_bytes: what gae_xw_fwd_workspace_bytes says for the shape (0: none needed)"""
    if xw_usable(m_aligned, ldm, n, K, J) and (xw_ws_bytes == 0 or ws_bytes >= xw_ws_bytes):
        return "xw", "xw_fwd_kernel"
    return gemm_kind(n, K, J, True, False, ldm, m_aligned, K, w_aligned, ws_floats=ws_bytes // 4, gemm_rows=gemm_rows,
                     linear_wlds=linear_wlds)


def atb_plan(n, O, I, atb_bf16=1):
    """(n_slots, rows_per_slot, slot_stride) of atb_plan(n, f_out, f_in)"""
    bf16 = bool(atb_bf16) and O <= 32 and I > 32
    cgroups = (I + 31) // 32 if I <= 32 else (I + 63) // 64 if bf16 else (I + 127) // 128
    tiles = max(cgroups, 1) * max((O + 31) // 32, 1)
    rows = max(((n * tiles + 207) // 208 + 127) // 128 * 128, 128)
    cap = max(min((32 << 20) // max(O * I, 1), 4096), 1)
    want = max(min((n + rows - 1) // rows, cap), 1)
    rps = max(((n + want - 1) // want + 127) // 128 * 128, 128)
    return max((n + rps - 1) // rps, 1), rps, (O * I + O + 3) // 4 * 4


def bwd_workspace_bytes(n, f_in, f_out, atb_bf16=1):
    """gae_linear_bwd_workspace_bytes"""
    slots, _, stride = atb_plan(n, f_out, f_in, atb_bf16)
    return (slots * stride * 4 + 255) // 256 * 256 + 256


def atb_kind(O, I, ldq, q_aligned, atb_bf16=1):
    """launch_atb on a 16-byte aligned workspace; I = 0: column sums only"""
    narrow = I <= 32
    I4 = (I + 3) // 4 * 4
    vec = not narrow and ldq % 4 == 0 and q_aligned and ldq >= I4 and I >= 4
    if atb_bf16 and vec and O <= 32:
        return "atb_bf16", f"atb_bf16_kernel<p3={int(atb_bf16 == 1)}>"
    if narrow:
        return "atb_narrow", "atb_partial_kernel<1, qvec=0>"
    return ("atb_vec", "atb_partial_kernel<4, qvec=1>") if vec else ("atb_scalar", "atb_partial_kernel<4, qvec=0>")


def bwd_kind(c):
    """gae_linear_bwd on a BWD case: the LAST product kernel of the call -- dM's when dM is wanted (after the weight
    gradient's), else the weight-gradient kernel"""
    n, f_in, f_out = c["n"], c["f_in"], c["f_out"]
    lddy, ldy, ldm = lead(f_out, c["ld_dY"]), lead(f_out, c["ld_Y"]), lead(f_in, c["ld_M"])
    if "dM" in c["want"]:
        pro = c["act"] == ACT_RELU
        return gemm_kind(n, f_out, f_in, False, pro, lddy, not c["mis_dY"], f_in, not c["mis_W"], ldy, not c["mis_Y"],
                         gemm_rows=c["gemm_rows"])
    return wgrad_kind(c)


def wgrad_kind(c):
    """the weight-gradient kernel of a BWD case (db alone: Q = dY, I = 0)"""
    if "dW" in c["want"]:
        return atb_kind(c["f_out"], c["f_in"], lead(c["f_in"], c["ld_M"]), not c["mis_M"], c["atb_bf16"])
    return atb_kind(c["f_out"], 0, lead(c["f_out"], c["ld_dY"]), not c["mis_dY"], c["atb_bf16"])


# ------------------------------------------------------------------ case tables
def _fwd(id, n, f_in, f_out, kind, mis_M=0, ld_M="w", mis_W=0, mis_Y=0, ld_Y="w", mis_b=0, ws=False, act=ACT_RELU,
         bias=True, gemm_rows=1, linear_wlds=1):
    return dict(id=id, n=n, f_in=f_in, f_out=f_out, kind=kind, mis_M=mis_M, ld_M=ld_M, mis_W=mis_W, mis_Y=mis_Y,
                ld_Y=ld_Y, mis_b=mis_b, ws=ws, act=act, bias=bias, gemm_rows=gemm_rows, linear_wlds=linear_wlds)


def _short_rows():
    """f_in <= 64: gemm_rows_kernel with the knob at 2, gemm_stream_kernel with it at 0, same operands"""
    shapes = [  # n, f_in, f_out, mis_M, ld_M, mis_W, mis_Y, ld_Y, act, bias
        (1, 1, 1, 0, "w", 0, 0, "w", ACT_IDENTITY, True),
        (31, 3, 7, 0, "4", 1, 1, "4", ACT_RELU, True),
        (32, 7, 16, 0, "odd", 0, 0, "odd", ACT_RELU, False),
        (33, 32, 32, 0, "w", 0, 1, "w", ACT_RELU, True),
        (63, 33, 33, 1, "4", 1, 0, "4", ACT_IDENTITY, True),
        (65, 39, 32, 0, "4", 0, 1, "odd", ACT_RELU, True),
        (129, 64, 33, 0, "w", 1, 0, "odd", ACT_RELU, True),
        (129, 64, 16, 1, "w", 0, 1, "4", ACT_IDENTITY, False),
    ]
    out = []
    for rows_knob, kind in ((2, "rows"), (0, "stream")):
        for n, fi, fo, mm, lm, mw, my, ly, act, bias in shapes:
            out.append(_fwd(f"{kind}-n{n}-k{fi}-j{fo}-M{'u' if mm else 'a'}ld{lm}-W{'u' if mw else 'a'}-"
                            f"Y{'u' if my else 'a'}ld{ly}", n, fi, fo, kind, mm, lm, mw, my, ly, 0, False, act, bias,
                            rows_knob))
    return out


FWD = _short_rows() + [
    # linear_fwd_pieces_kernel: 128 <= f_in <= 192 (wider aligned operands go to xw), rows of M whole 16-byte vectors
    _fwd("pieces-n33-k128-j16-Wa(wvec)", 33, 128, 16, "pieces", ld_Y="4"),
    _fwd("pieces-n33-k128-j16-Wu", 33, 128, 16, "pieces", mis_W=1, mis_Y=1),
    _fwd("pieces-n31-k130-j7-Mld4-Wa", 31, 130, 7, "pieces", ld_M="4", ld_Y="odd"),
    _fwd("pieces-n31-k130-j7-Mld4-Wu", 31, 130, 7, "pieces", ld_M="4", mis_W=1, act=ACT_IDENTITY),
    _fwd("pieces-n65-k192-j32-Wa(wvec)", 65, 192, 32, "pieces", mis_b=1),
    _fwd("pieces-n65-k192-j32-Mld4-Wu", 65, 192, 32, "pieces", ld_M="4", mis_W=1, mis_Y=1, ld_Y="odd"),
    _fwd("pieces-n1-k129-j1-Mld4", 1, 129, 1, "pieces", ld_M="4", bias=False),
    _fwd("pieces-n129-k2049-j32-Mld4-no-ws", 129, 2049, 32, "pieces", ld_M="4", mis_W=1),     # xw needs a workspace here
    # the same widths with rows of M that are not whole vectors: gemm_stream_kernel
    _fwd("stream-n33-k128-j16-Mu-Wa(bvec)", 33, 128, 16, "stream", mis_M=1),
    _fwd("stream-n31-k130-j7-Mldodd", 31, 130, 7, "stream", ld_M="odd", mis_W=1),
    # long rows, few row tiles: split-K with a workspace, unsplit without
    _fwd("split-n33-k520-j16-Mu-Wa(bvec)-ws", 33, 520, 16, "stream+split", mis_M=1, ws=True, mis_Y=1, ld_Y="odd"),
    _fwd("split-n33-k520-j16-Mu-Wu-ws", 33, 520, 16, "stream+split", mis_M=1, mis_W=1, ws=True, act=ACT_IDENTITY),
    _fwd("wlds-forced-n33-k520-j16-Mu-Wa(wvec)-ws", 33, 520, 16, "wlds", mis_M=1, ws=True, linear_wlds=2, ld_Y="4"),
    _fwd("wlds-forced-n65-k520-j7-Mldodd-Wu-ws", 65, 520, 7, "wlds", ld_M="odd", mis_W=1, ws=True, linear_wlds=2, mis_Y=1),
    _fwd("stream-n33-k520-j16-Mu-no-ws", 33, 520, 16, "stream", mis_M=1),
    _fwd("stream-n33-k520-j16-Mu-no-ws-wlds-forced", 33, 520, 16, "stream", mis_M=1, linear_wlds=2),   # 65 k-blocks > 64
    _fwd("wlds-default-n31-k2049-j7-Mldodd-ws", 31, 2049, 7, "wlds", ld_M="odd", ws=True, ld_Y="odd"),
    _fwd("wlds-default-n129-k2049-j32-Mu-Mld4-ws", 129, 2049, 32, "wlds", mis_M=1, ld_M="4", mis_W=1, ws=True),
    _fwd("split-n31-k2049-j7-Mldodd-ws-wlds0", 31, 2049, 7, "stream+split", ld_M="odd", ws=True, linear_wlds=0, mis_Y=1),
    _fwd("stream-n31-k2049-j7-Mldodd-no-ws", 31, 2049, 7, "stream", ld_M="odd"),
    _fwd("stream-n31-k2049-j7-Mldodd-no-ws-wlds-forced", 31, 2049, 7, "stream", ld_M="odd", linear_wlds=2),
    # linear_fwd_wlds_kernel forced on short rows: the avec instances
    _fwd("wlds-forced-n65-k64-j32-Ma-Wa", 65, 64, 32, "wlds", linear_wlds=2),
    _fwd("wlds-forced-n63-k39-j16-Mld4-Wa", 63, 39, 16, "wlds", ld_M="4", linear_wlds=2, ld_Y="4"),
    _fwd("wlds-forced-n129-k32-j1-Mu", 129, 32, 1, "wlds", mis_M=1, linear_wlds=2, act=ACT_IDENTITY),
    # f_out: 33 .. 64 two column tiles, 65 .. 128 four, above 128 gemm_kernel
    _fwd("stream-n65-k39-j65-Mld4", 65, 39, 65, "stream", ld_M="4", ld_Y="4"),
    _fwd("stream-n33-k130-j33-Mld4", 33, 130, 33, "stream", ld_M="4", mis_Y=1),
    _fwd("tiled-n129-k39-j130-Mld4(vec)", 129, 39, 130, "tiled", ld_M="4", ld_Y="odd"),
    _fwd("tiled-n65-k33-j130-Mu", 65, 33, 130, "tiled", mis_M=1, mis_W=1, mis_Y=1, ld_Y="4", act=ACT_IDENTITY),
    _fwd("tiled-n1-k7-j130", 1, 7, 130, "tiled", bias=False),
    # wide, aligned rows: gae_xw_fwd's kernel
    _fwd("xw-n33-k200-j16", 33, 200, 16, "xw", ld_Y="4"),
    _fwd("xw-n129-k2049-j32-Mld4-ws", 129, 2049, 32, "xw", ld_M="4", ws=True, mis_Y=1, ld_Y="odd"),
]


def _bwd(id, n, f_in, f_out, want, kind, act=ACT_RELU, atb_bf16=1, mis_dY=0, ld_dY="w", mis_Y=0, ld_Y="w", mis_M=0,
         ld_M="w", mis_W=0, mis_dM=0, ld_dM="w", gemm_rows=1):
    return dict(id=id, n=n, f_in=f_in, f_out=f_out, want=tuple(want.split("+")), kind=kind, act=act, atb_bf16=atb_bf16,
                mis_dY=mis_dY, ld_dY=ld_dY, mis_Y=mis_Y, ld_Y=ld_Y, mis_M=mis_M, ld_M=ld_M, mis_W=mis_W, mis_dM=mis_dM,
                ld_dM=ld_dM, gemm_rows=gemm_rows)


BWD = [
    # f_in <= 32: atb_partial_kernel<1>; every non-empty subset of {dW, db, dM}
    _bwd("narrow-n127-i7-o16-dW+db", 127, 7, 16, "dW+db", "atb_narrow", ld_M="4", ld_dY="4", ld_Y="odd"),
    _bwd("narrow-n128-i32-o32-dW", 128, 32, 32, "dW", "atb_narrow", act=ACT_IDENTITY),
    _bwd("narrow-n129-i1-o1-dW+db", 129, 1, 1, "dW+db", "atb_narrow"),
    _bwd("narrow-n257-i32-o33-db", 257, 32, 33, "db", "atb_narrow", mis_dY=1, mis_Y=1),
    _bwd("narrow-n33-i3-o7-dW+db-bf16=0", 33, 3, 7, "dW+db", "atb_narrow", atb_bf16=0, mis_M=1, ld_M="odd"),
    _bwd("dM-n129-i32-o16-dW+db+dM", 129, 32, 16, "dW+db+dM", "stream", ld_dM="4", ld_dY="4", ld_Y="4"),
    _bwd("dM-n65-i7-o33-dM", 65, 7, 33, "dM", "stream", mis_dY=1, ld_dM="odd", mis_dM=1),
    _bwd("dM-n63-i32-o32-db+dM-rows", 63, 32, 32, "db+dM", "rows", gemm_rows=2, act=ACT_IDENTITY),
    _bwd("dM-n31-i16-o7-dW+dM-rows", 31, 16, 7, "dW+dM", "rows", gemm_rows=2, ld_dY="odd", ld_Y="4", ld_dM="4"),
    # 33 <= f_in: atb_bf16_kernel where f_out <= 32 and the rows of M are whole vectors, else atb_partial_kernel<4>
    _bwd("bf16-n127-i33-o16-Mld4-dW+db", 127, 33, 16, "dW+db", "atb_bf16", ld_M="4"),
    _bwd("bf16-n128-i64-o32-dW+db", 128, 64, 32, "dW+db", "atb_bf16", act=ACT_IDENTITY),
    _bwd("bf16-n129-i65-o7-Mld4-dW", 129, 65, 7, "dW", "atb_bf16", ld_M="4", mis_dY=1, ld_dY="odd", ld_Y="4"),
    _bwd("bf16-n257-i130-o32-Mld4-dW+db", 257, 130, 32, "dW+db", "atb_bf16", ld_M="4", mis_Y=1),
    _bwd("bf16-n1-i64-o1-dW+db", 1, 64, 1, "dW+db", "atb_bf16"),
    _bwd("bf16=2-n129-i64-o16-dW+db", 129, 64, 16, "dW+db", "atb_bf16", atb_bf16=2),
    _bwd("bf16=2-n257-i130-o32-Mld4-dW+db", 257, 130, 32, "dW+db", "atb_bf16", atb_bf16=2, ld_M="4", act=ACT_IDENTITY),
    _bwd("vec-bf16=0-n127-i64-o16-dW+db", 127, 64, 16, "dW+db", "atb_vec", atb_bf16=0),
    _bwd("vec-bf16=0-n129-i33-o32-Mld4-dW+db", 129, 33, 32, "dW+db", "atb_vec", atb_bf16=0, ld_M="4", ld_dY="4"),
    _bwd("vec-bf16=0-n257-i130-o7-Mld4-dW", 257, 130, 7, "dW", "atb_vec", atb_bf16=0, ld_M="4", act=ACT_IDENTITY),
    _bwd("vec-n128-i65-o33-Mld4-dW+db", 128, 65, 33, "dW+db", "atb_vec", ld_M="4"),             # f_out > 32: no bf16 form
    _bwd("vec-n129-i128-o65-dW+db", 129, 128, 65, "dW+db", "atb_vec", mis_dY=1),
    _bwd("scalar-n127-i33-o16-dW+db", 127, 33, 16, "dW+db", "atb_scalar"),                        # ld = 33
    _bwd("scalar-n129-i64-o32-Mu-dW+db", 129, 64, 32, "dW+db", "atb_scalar", mis_M=1),
    _bwd("scalar-n257-i65-o33-Mldodd-dW", 257, 65, 33, "dW", "atb_scalar", ld_M="odd", atb_bf16=0),
    _bwd("scalar-n128-i130-o7-Mu-Mld4-dW+db", 128, 130, 7, "dW+db", "atb_scalar", mis_M=1, ld_M="4", act=ACT_IDENTITY),
    # dM = dYm W on wider layers: gemm_stream_kernel with B as [K, J] up to 128 columns, gemm_kernel above
    _bwd("dM-n129-i64-o32-dW+db+dM", 129, 64, 32, "dW+db+dM", "stream", ld_dM="odd"),
    _bwd("dM-n127-i65-o16-dY-ld4-dM", 127, 65, 16, "dM", "stream", ld_dY="4", ld_Y="4", mis_W=1, ld_dM="4"),
    _bwd("dM-n33-i33-o130-dW+dM", 33, 33, 130, "dW+dM", "stream", act=ACT_IDENTITY, mis_dM=1),
    _bwd("dM-n257-i130-o32-dW+db+dM-tiled", 257, 130, 32, "dW+db+dM", "tiled", ld_M="4", ld_dM="4"),
    _bwd("dM-n65-i130-o7-dYu-db+dM-tiled", 65, 130, 7, "db+dM", "tiled", mis_dY=1, ld_dM="odd", mis_dM=1),
    _bwd("dM-n129-i130-o33-dM-tiled", 129, 130, 33, "dM", "tiled", ld_dY="4", ld_Y="odd", act=ACT_IDENTITY),
]

# gae_x_linear_bwd_partials against gae_linear_bwd: (n, f_in, f_out, want_dW, want_db, act, atb_bf16, mis_M, ld_M)
PARTIALS = [
    (127, 7, 16, 1, 1, ACT_RELU, 1, 0, "4"),
    (129, 32, 32, 1, 1, ACT_IDENTITY, 1, 1, "w"),
    (257, 64, 16, 1, 1, ACT_RELU, 1, 0, "w"),
    (257, 130, 7, 1, 0, ACT_RELU, 0, 0, "4"),
    (129, 65, 33, 1, 1, ACT_RELU, 1, 0, "odd"),
    (257, 33, 16, 0, 1, ACT_RELU, 1, 0, "w"),
]

SHAPES = sorted({(c["n"], c["f_in"], c["f_out"]) for c in FWD + BWD})


# ------------------------------------------------------------------ inputs
def draw(seed, *shape):
    """N(0, 1) fp32, a few exact zeros"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape).astype(np.float32)
    x[rng.random(shape) < 0.03] = 0.0
    return x


def draw_mask(seed, *shape):
    """a stored activation Y: about half the entries positive, the rest +0, -0 and a few negative values (a kernel
    that tests Y >= 0, Y != 0 or the sign bit reads another mask)"""
    rng = np.random.default_rng(seed)
    y = np.maximum(rng.standard_normal(shape), 0.0).astype(np.float32)
    u = rng.random(shape)
    y[(y == 0) & (u < 0.3)] = np.float32(-0.0)
    y[(y == 0) & (u > 0.9)] = np.float32(-1.5)
    return y
