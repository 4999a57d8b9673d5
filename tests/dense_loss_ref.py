"""Reference for the dense loss chain gae_decoder_dense -> gae_csr_to_dense -> gae_bce_logits -> gae_decoder_dense_bwd
(csrc/dense.hip, csrc/csr_build.hip, csrc/bce_dense.hip), numpy only: float64 results, a derived rounding bound per
output element, a host restatement of which kernel a decoder call takes (written from gae_decoder_dense,
gae_decoder_dense_bwd, dispatch_gemm and launch_atb; used to pick and to label cases, never to excuse one) and the case
tables that tests/test_dense_loss_ref_cpu.py and tests/test_gpu_dense_loss_abi.py share.  The arena, lead(),
worst_element(), wgrad_bound(), atb_plan(), atb_kind() and draw() are tests/dense_ref.py's.

u = 2^-24 is the unit roundoff of fp32: one rounded operation has relative error at most u.

Decoder.  The kernels form zt = fl32(z m) with ONE fp32 multiply before any product (gemm_kernel's PRO_MUL_MASK /
MASK_B staging, atb_partial_kernel's and atb_bf16_kernel's `av *= st.m`), so the references start from that rounded
zt (zt = z without a mask) and what is left is summation error:
  forward   out = zt zt^T, contraction length d:  |err_ij| <= (d + 4) u sum_k |zt_ik| |zt_jk|   (any order of fp32 adds
            of exact products; dense_ref.linear_fwd's bound)
  backward  dZ = ((G zt) + (G^T zt)) (.) m.  Term 1 (G zt, an fp32 GEMM of length n) errs by (n + 4) u |G| |zt|.  Term 2
            (G^T zt = (zt^T G)^T, launch_atb's partial slots, added in slot order) errs by w |G|^T |zt| with
            w = dense_ref.wgrad_bound(n, atb_bf16) when atb_bf16_kernel ran and (n + 4) u otherwise.
            reduce_slots_transposed_kernel then adds the two terms (one rounding, relative to |t1 + t2|) and multiplies
            by the mask (one more): 4 u (|G| |zt| + |G|^T |zt|) covers both and their second-order products.  All of it
            scales with |m|.

BCE (bce_elem of csrc/bce_dense.hip).  Labels y in {0, 1, 2} and pos_weight in {1, 0.5, 37.5, 1023}: a = 1 - y and
lw = 1 + (pw - 1) y are then exact in fp32 and lw >= 0 (lw = 0 only for pw = 0.5, y = 2, where every lw term vanishes
exactly).  With E = exp(-|x|):
      l = a x + lw softplus(-x),    softplus(-x) = max(-x, 0) + log1p(E)
      g = (a - lw sigmoid(-x)) inv, sigmoid(-x) = E / (1 + E) for x >= 0, 1 / (1 + E) for x < 0,   inv = 1 / (n m)
ONE ASSUMPTION: the fast __expf returns e = E (1 + de) with |de| <= (2 + 2 |x|) u (an exp2 of a rounded product
x log2(e): the product's rounding error is multiplied by |x|).  Beside it log1pf is allowed 2 ulp = 4 u relative and the
fp32 division 1 ulp = 2 u (the library is built without fast-math flags, where hipcc rounds the division correctly:
u).  Results that underflow (E below 2^-126, |x| > 87.3) may be flushed to zero: an
absolute error below 2^-126, nothing next to the absolute bounds below.
  sigmoid:  d/dE of both branches is 1 / (1 + E)^2 in magnitude, so e's error moves sigmoid(-x) by at most
            E (2 + 2 |x|) u <= 2 u  (E (1 + |x|) <= 1 for every x).  The add 1 + e and the division are 3 u relative to a
            value <= 1/2 (x >= 0) or < 1 (x < 0).  Together: |sn - sigmoid(-x)| <= 5 u for every finite x.
  g:        lw sn: 5 u lw from sn, u lw from the multiply.  a - lw sn: u (|a| + lw).  Times float(inv) (u) and the
            multiply (u): 2 u (|a| + lw).  Sum: inv u (9 lw + 3 |a|) <= inv u (16 lw + 4 |a|), the bound used.
  l:        log1p(e) against log1p(E): e's error moves it by E (2 + 2 |x|) u / (1 + E) <= 2 u (1 + |x|) E; log1pf's own
            error is 4 u log1p(E) <= 4 u sp.  The add of max(-x, 0), the multiply by lw and the final add each cost
            u (their result), the product a x costs u |a x| twice (its rounding and the final add):
            |err| <= 2 u |a x| + lw u (2 (1 + |x|) E + 7 sp) <= 8 u (|a x| + lw (sp + (1 + |x|) E)), the bound used.
  loss:     the terms are added in fp64 (2^-53 relative per add: nothing), scaled by the fp64 inv and rounded to fp32
            once: inv sum(term bounds) + 2 u |loss|.
The bounds are absolute on the scale of lw and |a|: they see a gradient that is zeroed, 2 % off, or taken from the wrong
branch, not the last bits of a gradient that is itself 1e-18.

csr_to_dense: integer counts (duplicates add), compared exactly."""
import numpy as np

import dense_ref as R

U24 = R.U24
LABELS = (0.0, 1.0, 2.0)
POS_WEIGHTS = (1.0, 0.5, 37.5, 1023.0)
LADDER = (0.0, 1e-40, 1e-7, 0.5, 16.6, 17.4, 40.0, 87.0, 88.8, 104.0, 1e4)   # each with both signs
BCE_GRID_ELEMS = 2048 * 256          # kBlocks * 256 threads: above it the grid-stride loop takes another trip


def _f64(x):
    return np.asarray(x, np.float64)


# ------------------------------------------------------------------ decoder
def masked_z(Z, mask):
    """zt = fl32(z m): one fp32 multiply; z itself without a mask"""
    Z = np.asarray(Z, np.float32)
    if mask is None:
        return Z
    zt = Z * np.asarray(mask, np.float32)
    assert zt.dtype == np.float32
    return zt


def decoder_dense(Z, mask):
    """(out, bound) of out = zt zt^T"""
    zt = _f64(masked_z(Z, mask))
    d = zt.shape[1]
    return zt @ zt.T, (d + 4) * U24 * (np.abs(zt) @ np.abs(zt).T)


def decoder_dense_bwd(G, Z, mask, atb_bf16=0):
    """(dZ, bound) of dZ = ((G zt) + (G^T zt)) (.) m.  atb_bf16: the form of atb_bf16_kernel when the call's kind is
    atb_bf16 (1: three pieces, 2: two), 0 when an exact-fp32 kernel ends the call"""
    G, zt = _f64(G), _f64(masked_z(Z, mask))
    n = G.shape[0]
    m = np.ones_like(zt) if mask is None else _f64(np.asarray(mask, np.float32))
    t1, t2 = G @ zt, G.T @ zt
    m1, m2 = np.abs(G) @ np.abs(zt), np.abs(G).T @ np.abs(zt)
    w = R.wgrad_bound(n, atb_bf16) if atb_bf16 else (n + 4) * U24
    return (t1 + t2) * m, np.abs(m) * ((n + 4) * U24 * m1 + w * m2 + 4 * U24 * (m1 + m2))


# ------------------------------------------------------------------ BCE
def bce_terms(x, y, pw):
    """float64 (l, g_unscaled, a, lw, sp, E) per element of float64 logits x"""
    x, y = _f64(x), _f64(y)
    a, lw = 1.0 - y, 1.0 + (float(pw) - 1.0) * y
    E = np.exp(-np.abs(x))
    sp = np.maximum(-x, 0.0) + np.log1p(E)
    sn = np.where(x >= 0, E / (1.0 + E), 1.0 / (1.0 + E))
    return a * x + lw * sp, a - lw * sn, a, lw, sp, E


def bce_logits(x, y, pw):
    """dict: loss, loss_bound (scalars), grad, grad_bound ([n, m]), terms, term_bound ([n, m], unscaled) of the mean
    weighted BCE on fp32 logits x and labels y in {0, 1, 2}"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    assert x.shape == y.shape and np.isin(y, LABELS).all() and float(pw) in POS_WEIGHTS
    l, g, a, lw, sp, E = bce_terms(x, y, pw)
    assert (lw >= 0).all()
    inv = 1.0 / x.size if x.size else 0.0
    tb = 8 * U24 * (np.abs(a * _f64(x)) + lw * (sp + (1.0 + np.abs(_f64(x))) * E))
    loss = float(l.sum() * inv)
    return dict(loss=loss, loss_bound=float(inv * tb.sum() + 2 * U24 * abs(loss)), grad=g * inv,
                grad_bound=inv * U24 * (16 * lw + 4 * np.abs(a)), terms=l, term_bound=tb)


def old_rel_err(a, b):
    """the measure test_bce_logits_kernel uses: max |a - b| / max(1, max |b|)"""
    return float(np.abs(_f64(a) - _f64(b)).max() / max(1.0, float(np.abs(_f64(b)).max())))


def parity_bce_inputs():
    """the logits, labels and pos_weight of tests/test_gpu_parity.py::test_bce_logits_kernel"""
    rng = np.random.default_rng(3)
    n, m = 301, 517
    x = rng.standard_normal((n, m)).astype(np.float32) * 4
    y = ((rng.random((n, m)) < 0.02) * rng.integers(1, 3, (n, m))).astype(np.float32)
    return x, y, 37.5


# ------------------------------------------------------------------ csr_to_dense
def csr_to_dense(indptr, indices, n_rows, n_cols):
    out = np.zeros((n_rows, n_cols), np.int64)
    for r in range(n_rows):
        np.add.at(out[r], np.asarray(indices[indptr[r]:indptr[r + 1]], np.int64), 1)
    return out


# ------------------------------------------------------------------ which kernel a decoder call takes
def fwd_kind(c):
    """gae_decoder_dense: launch_gemm<4, BT, PRO, MASK_B> whatever n and d are"""
    ldz = R.lead(c["d"], c["ld_Z"])
    if c["mask"]:
        vec = ldz % 4 == 0 and not c["mis_Z"] and not c["mis_m"]
        return "tiled", f"gemm_kernel<4, bt=1, pro=mul_mask, mask_b=1, vec_a={int(vec)}>"
    return "tiled", f"gemm_kernel<4, bt=1, pro=none, mask_b=0, vec_a={int(ldz % 4 == 0 and not c['mis_Z'])}>"


def ld_of(width, kind):
    """a case's leading dimension: one of dense_ref.lead's kinds or the value itself"""
    return kind if isinstance(kind, int) else R.lead(width, kind)


def bwd_kind(c, mask):
    """gae_decoder_dense_bwd: (kind that ends the call = launch_atb's for term 2 with O = d, I = n, Q = G;
    its instance; the instance of term 1, for the test id only)"""
    n, d = c["n"], c["d"]
    ldg, ldz = ld_of(n, c["ld_G"]), R.lead(d, c["ld_Z"])
    kind, inst = R.atb_kind(d, n, ldg, not c["mis_G"], c["atb_bf16"])
    if mask:            # dispatch_gemm<false, PRO_NONE, true>: MASK_B never takes the stream kernel
        nt = 1 if d <= 32 else 2 if d <= 64 else 4
        term1 = f"gemm_kernel<{nt}, bt=0, mask_b=1, vec_a={int(ldg % 4 == 0 and not c['mis_G'])}>"
    else:
        k1, i1 = R.gemm_kind(n, n, d, False, False, ldg, not c["mis_G"], ldz, not c["mis_Z"])
        term1 = f"{k1}: {i1}"
    return kind, inst, term1


def bwd_workspace_bytes(n, d, atb_bf16=1):
    """gae_decoder_dense_bwd_workspace_bytes: the slots of atb_plan(n, O = d, I = n) and 256 bytes"""
    return R.bwd_workspace_bytes(n, n, d, atb_bf16)


BCE_WORKSPACE_BYTES = 2048 * 8      # gae_bce_logits_workspace_bytes: one double per block of the largest grid


# ------------------------------------------------------------------ case tables
def _fwd(n, d, mask, ld_Z="w", mis_Z=0, mis_m=0, ld_out="w", mis_out=0):
    c = dict(n=n, d=d, mask=mask, ld_Z=ld_Z, mis_Z=mis_Z, mis_m=mis_m, ld_out=ld_out, mis_out=mis_out, kind="tiled")
    c["id"] = (f"n{n}-d{d}-{'mask' if mask else 'nomask'}-Z{'u' if mis_Z else 'a'}ld{ld_Z}"
               f"{'-mu' if mask and mis_m else ''}-out{'u' if mis_out else 'a'}ld{ld_out}")
    return c


FWD = [
    _fwd(1, 1, 1),
    _fwd(1, 130, 0, "4", ld_out="odd", mis_out=1),
    _fwd(31, 3, 1, "odd", mis_Z=1, ld_out="4"),
    _fwd(31, 16, 0, ld_out="4", mis_out=1),
    _fwd(31, 65, 0, "odd"),
    _fwd(128, 32, 1),                                        # whole tiles, float4 staging of Z and mask
    _fwd(128, 33, 0, "odd", ld_out="odd"),
    _fwd(129, 39, 1, "4", ld_out="4"),                       # VEC_A with a K tail (ld 40): the scalar tail of a vector row
    _fwd(129, 39, 0, "4", mis_out=1),
    _fwd(129, 16, 1, mis_m=1, ld_out="odd"),                 # the mask alone off a 16-byte boundary: scalar staging
    _fwd(129, 65, 1, "4", mis_Z=1, mis_m=1),
    _fwd(257, 1, 1, "4"),                                    # one column on ld 4: a vector row that is all tail
    _fwd(257, 32, 0, mis_Z=1, ld_out="odd"),
    _fwd(257, 130, 1, "4", ld_out="4", mis_out=1),
]


def _bwd(n, d, kind, atb_bf16=1, ld_G="w", mis_G=0, ld_Z="w", mis_Z=0, mis_m=0, ld_dZ="w", mis_dZ=0):
    c = dict(n=n, d=d, kind=kind, atb_bf16=atb_bf16, ld_G=ld_G, mis_G=mis_G, ld_Z=ld_Z, mis_Z=mis_Z, mis_m=mis_m,
             ld_dZ=ld_dZ, mis_dZ=mis_dZ)
    c["id"] = (f"{kind[4:]}-n{n}-d{d}{'' if atb_bf16 == 1 else '-bf16=%d' % atb_bf16}-G{'u' if mis_G else 'a'}ld{ld_G}-"
               f"Z{'u' if mis_Z else 'a'}ld{ld_Z}-dZ{'u' if mis_dZ else 'a'}ld{ld_dZ}")
    return c


BWD = [
    # n <= 32: atb_partial_kernel<1>
    _bwd(1, 16, "atb_narrow", ld_dZ="4"),
    _bwd(7, 65, "atb_narrow", ld_G="odd", ld_Z="odd", mis_dZ=1),
    _bwd(32, 33, "atb_narrow", mis_G=1, ld_Z="4", ld_dZ="odd"),
    # d <= 32, n > 32, rows of G whole 16-byte vectors: atb_bf16_kernel
    _bwd(132, 16, "atb_bf16", ld_dZ="4"),                            # a contiguous batch of 132 nodes
    _bwd(129, 7, "atb_bf16", ld_G=132, ld_Z="odd", ld_dZ="odd"),     # ldg > n: the column tail reads NaN pads
    _bwd(257, 32, "atb_bf16", ld_G=260, mis_Z=1, mis_dZ=1),          # three slots
    _bwd(260, 1, "atb_bf16", ld_Z="4", mis_m=1),
    _bwd(132, 16, "atb_bf16", atb_bf16=2, ld_Z="4", ld_dZ="odd"),
    _bwd(257, 32, "atb_bf16", atb_bf16=2, ld_G=260, ld_dZ="4"),
    # d > 32 (or the knob at 0), rows of G whole vectors: atb_partial_kernel<4, qvec>
    _bwd(132, 33, "atb_vec", ld_Z="4", ld_dZ="4"),
    _bwd(129, 65, "atb_vec", ld_G=132, ld_dZ="odd"),
    _bwd(260, 130, "atb_vec", ld_Z="odd", mis_dZ=1),
    _bwd(132, 16, "atb_vec", atb_bf16=0),
    # rows of G that are no whole vectors: atb_partial_kernel<4> with scalar loads
    _bwd(129, 16, "atb_scalar", ld_dZ="4"),                          # a contiguous batch of 129 nodes
    _bwd(131, 48, "atb_scalar", ld_Z="4", mis_Z=1, ld_dZ="odd"),
    _bwd(257, 130, "atb_scalar", ld_G=260, mis_G=1, ld_dZ="4"),      # ld 260, base one float off
]


DECODER_SHAPES = sorted({(c["n"], c["d"]) for c in FWD + BWD})


def decoder_inputs(n, d):
    """(Z, mask, G): N(0, 1) embeddings with a few exact zeros, an inverted-dropout mask (0 or 1 / 0.9: a rounded
    multiplier, so z m does round) and a non-symmetric upstream gradient"""
    rng = np.random.default_rng(1000 * n + d)
    mask = ((rng.random((n, d)) >= 0.1) / 0.9).astype(np.float32)
    G = R.draw(33, n, n)
    assert n < 4 or not np.array_equal(G, G.T)
    return R.draw(31, n, d), mask, G


def _bce(rows, cols, pw, mode="grad", ld_x="w", mis_x=0, ld_y="w", mis_y=0, ld_g="w", mis_g=0, ladder=False):
    c = dict(rows=rows, cols=cols, pw=pw, mode=mode, ld_x=ld_x, mis_x=mis_x, ld_y=ld_y, mis_y=mis_y, ld_g=ld_g,
             mis_g=mis_g, ladder=ladder)
    c["id"] = (f"{'ladder' if ladder else 'r%d-c%d' % (rows, cols)}-pw{pw:g}-{mode}-x{'u' if mis_x else 'a'}ld{ld_x}-"
               f"y{'u' if mis_y else 'a'}ld{ld_y}" + (f"-g{'u' if mis_g else 'a'}ld{ld_g}" if mode == "grad" else ""))
    return c


# mode: "grad" a gradient buffer of its own, "null" grad = NULL, "alias" grad = logits (compared bit for bit with a
# separate-buffer call on the same operands)
BCE = [
    _bce(1, 1, 1.0),
    _bce(1, 1, 37.5, "alias", mis_x=1),
    _bce(1, 255, 0.5, ld_x="4", ld_y="odd", mis_g=1),
    _bce(16, 16, 1023.0, ld_x="odd", ld_y="4", mis_g=1),
    _bce(16, 16, 37.5, "null", ld_x="4", mis_y=1),
    _bce(1, 257, 37.5, mis_x=1, ld_y="4", ld_g="odd"),
    _bce(257, 1, 1.0, ld_x="4", ld_y="odd", mis_g=1),
    _bce(257, 1, 0.5, "alias", ld_x="odd", mis_y=1),
    _bce(301, 517, 37.5, ld_x="4", ld_y="w", ld_g="odd"),
    _bce(301, 517, 37.5, "alias", ld_x="odd", ld_y="4", mis_x=1),
    _bce(301, 517, 1023.0, "null", mis_x=1, ld_y="odd"),
    _bce(733, 719, 37.5, ld_x="4", ld_y="odd", mis_y=1, ld_g="w", mis_g=1),      # 527 027 > 2048 * 256: a second trip
    _bce(733, 719, 0.5, "alias", ld_y="4"),
] + [_bce(3, 2 * len(LADDER), pw, "grad", ld_x="4", ld_y="odd", mis_g=1, ladder=True) for pw in POS_WEIGHTS] \
  + [_bce(3, 2 * len(LADDER), 1023.0, "alias", mis_x=1, ladder=True)]


def bce_inputs(c):
    """(logits, labels) of a BCE case: the value ladder crossed with y = 0, 1, 2 (one row per label), else 4 N(0, 1)
    logits with about 2 % positive labels (1 or 2)"""
    if c["ladder"]:
        v = np.array(LADDER, np.float32)
        x = np.concatenate([v, -v])
        assert np.signbit(x[len(v)]) and x[len(v)] == 0 and x[1] != 0       # -0 and a subnormal are on the ladder
        return np.tile(x, (3, 1)), np.repeat(np.array(LABELS, np.float32)[:, None], x.size, 1)
    rng = np.random.default_rng(c["rows"] * 1000 + c["cols"])
    shape = (c["rows"], c["cols"])
    x = (4 * rng.standard_normal(shape)).astype(np.float32)
    y = ((rng.random(shape) < 0.02) * rng.integers(1, 3, shape)).astype(np.float32)
    if x.size > 1:
        y.reshape(-1)[:2] = (1.0, 2.0)            # both positive labels occur whatever the draw
    return x, y


def _csr(id, n_rows, n_cols, ld, rows):
    """rows: {row: [columns]}"""
    indptr = np.zeros(n_rows + 1, np.int32)
    for r, cols in rows.items():
        indptr[r + 1] = len(cols)
    indptr = np.cumsum(indptr).astype(np.int32)
    indices = np.array([c for r in sorted(rows) for c in rows[r]], np.int32)
    assert indices.size == indptr[-1] and (indices.size == 0 or (0 <= indices.min() and indices.max() < n_cols))
    return dict(id=id, n_rows=n_rows, n_cols=n_cols, ld=ld, indptr=indptr, indices=indices)


def _csr_cases():
    rng = np.random.default_rng(7)
    return [
        _csr("5x9-ld9-empty-rows", 5, 9, 9, {1: [0, 8, 3], 3: [8, 8, 1]}),
        _csr("5x9-ld12-70-copies", 5, 9, 12, {0: [2], 4: [7] * 70 + [0]}),
        _csr("5x9-ld11-no-edges", 5, 9, 11, {}),
        _csr("130x1-ld1", 130, 1, 1, {r: [0] * int(k) for r, k in enumerate(rng.integers(0, 4, 130))}),
        _csr("130x1-ld3-70-copies", 130, 1, 3, {0: [0], 64: [0] * 70, 129: [0, 0]}),
        _csr("1x130-ld131-row-of-200", 1, 130, 131, {0: rng.integers(0, 130, 200).tolist()}),
        _csr("1x130-ld130", 1, 130, 130, {0: [129, 0, 64, 64]}),
    ]


CSR = _csr_cases()

# the Python chain: (n, d, entry point); 129 and 132 are the two gradient kernels a real batch alternates between
CHAIN = [(129, 16, "dense"), (132, 16, "dense"), (131, 65, "decoder_bce")]


def chain_inputs(n, d):
    """(Z, mask, src, dst) with duplicate edges"""
    rng = np.random.default_rng(100 * n + d)
    Z = (0.3 * rng.standard_normal((n, d))).astype(np.float32)
    mask = ((rng.random((n, d)) >= 0.1) / 0.9).astype(np.float32)
    src, dst = rng.integers(0, n, 5 * n), rng.integers(0, n, 5 * n)
    src[:8], dst[:8] = src[8:16], dst[8:16]
    return Z, mask, src.astype(np.int64), dst.astype(np.int64)


def chain_ref(Z, mask, src, dst):
    """float64 (loss, dZ, pos_weight, A) of mean BCE((Z m)(Z m)^T, A, pw) with A[dst, src] += 1 and
    pw = (n^2 - nnz) / nnz (train_inductive.py:44-48); the multiply z m is exact in float64 here: the chain is held to a
    norm-wise bound, not to the kernels' own rounding"""
    n = Z.shape[0]
    A = np.zeros((n, n), np.int64)
    np.add.at(A, (dst, src), 1)
    pw = (float(n) * n - src.size) / src.size
    zt = _f64(Z) * _f64(mask)
    l, g = bce_terms(zt @ zt.T, A, pw)[:2]
    g = g / (n * n)
    return float(l.mean()), ((g + g.T) @ zt) * _f64(mask), pw, A
