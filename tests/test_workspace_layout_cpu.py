"""The workspace layouts do not move: every size query, and the pointers gae_x_decoder_bce_prep_layout exports, keep the
values of the commit BEFORE the layouts were restated through gae::Carver (one walk per family, run for the size and for
the pointers).  The size queries are host code: no GPU.  Offsets decide alignment and the size class of the workspace
cache a call lands in, so a changed number here is a behaviour change.

The expected numbers were evaluated with the library built from commit 1534cfe ("Random forest head on the device"),
default knob values, and pasted in; they never come from the tree under test."""
import ctypes

import pytest


def _lib():
    import __graft_entry__ as ge
    ge.build()
    from gae_dgl_amd import _lib
    return _lib


def _sampled_bytes(L, n, n_local, d):
    out = ctypes.c_int64(-1)
    rc = L.load().gae_decoder_bce_sampled(None, None, d, n, d, 0, n_local, 1, None, None, None, None, 1.0, 0.0, 0, 0, None,
                                          None, None, d, None, None, ctypes.byref(out), None)
    assert rc == 0
    return out.value


def _threshold_bytes(L, entry, n, d, splits):
    out = ctypes.c_int64(-1)
    tail = (None,) if entry == "gae_decoder_threshold_count" else (None, None, None, 0)
    rc = getattr(L.load(), entry)(None, d, n, d, 0.0, None, 0, 0, None, None, 0, splits, *tail, None, ctypes.byref(out), None)
    assert rc == 0
    return out.value


def _spmm_bytes(L, n_heavy, n_segments, n_virtual, F):
    plan = L.SpmmPlan()
    plan.n_heavy, plan.n_segments, plan.vh_n_virtual = n_heavy, n_segments, n_virtual
    return L.load().gae_spmm_workspace_bytes(ctypes.byref(plan), F)


def _embed_bwd_bytes(L, f_in, widths, n_out):
    return L.load().gae_embed_graphs_bwd_workspace_bytes(f_in, len(widths), (ctypes.c_int64 * len(widths))(*widths), n_out)


def _prep_layout(L, n, d):
    nbytes = L.load().gae_decoder_bce_workspace_bytes(n, n, d)
    raw = ctypes.create_string_buffer(nbytes + 256)
    base = (ctypes.addressof(raw) + 255) // 256 * 256                  # a 256-byte-aligned host buffer
    prep = L.BcePrep()
    assert L.load().gae_x_decoder_bce_prep_layout(n, d, ctypes.c_void_p(base), nbytes, ctypes.byref(prep)) == 0
    return (prep.Zt - base, prep.Zhi - base, prep.Zlo - base, prep.colsum_partial - base, prep.scal - base,
            prep.all_pairs, prep.max_blocks, prep.DP)


# (query, arguments) -> the parent commit's answer
SIZES = {
    "gae_decoder_bce_workspace_bytes": {
        (100, 100, 16): 28928,                       # plain grid
        (2708, 2708, 16): 4212480,
        (5119, 5119, 16): 9602048,
        (5120, 5120, 16): 17621248,                  # the balanced symmetric schedule starts here
        (8192, 8192, 16): 23995136,
        (19717, 19717, 16): 71297280,
        (32768, 32768, 16): 160969728,
        (65536, 65536, 16): 665969664,               # balanced off
        (19717, 5000, 16): 12781312,                 # a row window: no symmetric form
        (19717, 19717, 32): 41053440,
        (3000, 3000, 33): 20174080,                  # KS 3 becomes 4
        (3000, 3000, 64): 20174080,
        (100, 200, 16): -2,                          # n_local > n
    },
    "gae_kmeans_workspace_bytes": {
        (1, 1, 1): 3840, (256, 64, 256): 272896, (19717, 16, 7): 232704, (249455, 48, 64): 7442944,
        (5, 16, 7): -2,                              # more centres than rows
    },
    "gae_knn_workspace_bytes": {
        (1, 1, 1, 1, 0): 768, (1128, 1128, 48, 10, 0): 456192, (19717, 19717, 16, 64, 16): 161601024,
        (7, 249455, 256, 64, 0): 1055488,
    },
    "gae_tanimoto_knn_workspace_bytes": {            # from commit 6aa1ace, which added K34 (m, n, n_words, k, splits)
        (1, 1, 1, 1, 0): 768, (1128, 1128, 32, 10, 0): 456192, (19717, 19717, 32, 64, 16): 161601024,
        (7, 249455, 64, 64, 0): 1055488, (4096, 249455, 32, 64, 0): 34552576,
    },
    "gae_ridge_workspace_bytes": {(0, 1, 1, 1): 512, (1128, 48, 1, 5): 102400, (249455, 128, 8, 32): 76153856},
    "gae_forest_workspace_bytes": {
        (1, 1, 1, 1, 1, 1, 2): 4352,
        (1128, 48, 1, 100, 1128, 12, 64): 16786176,
        (19717, 16, 8, 1024, 8193, 16, 256): 6478001152,
        (249455, 48, 1, 100, 249455, 12, 64): 360152320,
    },
    "gae_spmm_plan_scratch_bytes": {
        (0, 0, 0, 0, 64): 23552, (19717, 19717, 0, 0, 256): 182528, (1 << 20, 1 << 20, 37, 5000000, 1024): 8629248,
    },
    "gae_linear_bwd_workspace_bytes": {(2708, 1433, 32): 1468672, (19717, 500, 32): 1667584, (3327, 3703, 32): 1896704},
    "gae_linear_fwd_workspace_bytes": {(2708, 1433, 32): 3466240, (19717, 500, 32): 0, (3327, 3703, 32): 3406848},
    "gae_decoder_dense_bwd_workspace_bytes": {(2708, 16): 867328, (19717, 16): 1262336},
    "gae_csr_from_coo_workspace_bytes": {(0, 0): 512, (88648, 19717): 1419008},
    "gae_decoder_bce_graphs_workspace_bytes": {(0, 0, 0, 1): 64, (250000, 10000, 64, 16): 160064, (19717, 1, 19717, 16): 2552},
    "gae_xw_fwd_workspace_bytes": {(1, 64, 1, 0): 0, (2708, 1433, 32, 0): 1733120, (3327, 3703, 32, 1): 1703424},
    "gae_xw_wgrad_workspace_bytes": {(1, 1, 0): 8704, (2708, 1433, 0): 2106624, (3327, 3703, 1): 3832064},
}
SAMPLED = {(1, 1, 1): 62720, (2708, 2708, 16): 306432, (100000, 25000, 33): 14913792}
THRESHOLD = {(0, 1, 0): 512, (19717, 16, 0): 1657600, (19717, 16, 16): 3788544}       # (n, d, splits), both entry points
SPMM = {(0, 0, 0, 32): 0, (1, 1, 0, 1): 256, (120, 4000, 0, 32): 512000, (0, 0, 700, 16): 44800,
        (120, 4001, 700, 30): 601856}                                                  # (n_heavy, n_segments, n_virtual, F)
EMBED_BWD = {(1, (1,), 0): 32, (39, (32, 16), 100000): 14840064}                       # (f_in, widths, n_out)
PREP_LAYOUT = {                                      # (n, d) -> the five offsets, all_pairs, max_blocks, DP
    (2708, 16): (3812864, 3986176, 4072960, 4159744, 4203840, 7452416.0, 171, 16),
    (19717, 16): (17666560, 18928640, 19559680, 20190720, 20506944, 388760089.0, 1234, 16),
    (3000, 33): (18432000, 19200000, 19584000, 19968000, 20162816, 9024000.0, 189, 64),
}


@pytest.mark.parametrize("query", sorted(SIZES))
def test_size_queries_keep_their_values(query):
    fn = getattr(_lib().load(), query)
    got = {args: fn(*args) for args in SIZES[query]}
    assert got == SIZES[query]


def test_null_workspace_queries_keep_their_values():
    L = _lib()
    assert {a: _sampled_bytes(L, *a) for a in SAMPLED} == SAMPLED
    for entry in ("gae_decoder_threshold_count", "gae_decoder_threshold_fill"):
        assert {a: _threshold_bytes(L, entry, *a) for a in THRESHOLD} == THRESHOLD, entry
    assert {a: _spmm_bytes(L, *a) for a in SPMM} == SPMM
    assert {a: _embed_bwd_bytes(L, *a) for a in EMBED_BWD} == EMBED_BWD


@pytest.mark.parametrize("shape", sorted(PREP_LAYOUT))
def test_bce_prep_layout_keeps_its_offsets(shape):
    assert _prep_layout(_lib(), *shape) == PREP_LAYOUT[shape]
