"""Neighbourhood link-prediction baselines (K35 gae_neighbour_pairs, K36 gae_neighbour_topk): common neighbours, Jaccard,
Adamic-Adar, resource allocation and preferential attachment of a symmetric graph -- the rows a link-prediction table is
compared against first.  No n x n two-hop matrix is formed and the kernels accumulate integers only: Adamic-Adar and
resource allocation are sums of fixed-point weights (32 fraction bits) from a host table over the degrees, so every score has
the same bits run to run and equals the numpy restatement of the header comment bit for bit.

Part of the package gae_dgl_amd.ops; names are resolved through the package namespace (`_ops.<name>`) at call time."""
import collections

import numpy as np
import torch

from .. import _lib
from .._lib import GaeHipError
from ._base import _gpu, _on_device, _ptr, _stream, _timed, _ws_bytes

__all__ = ['NeighbourScores', 'NeighbourTopK', 'NEIGHBOUR_SCALE_BITS', 'NEIGHBOUR_TABLE_SLOTS', 'NEIGHBOUR_KINDS',
           'neighbour_weight_table', 'neighbour_weights', 'neighbour_scores', 'neighbour_topk', 'neighbour_last_routes']

NEIGHBOUR_SCALE_BITS, NEIGHBOUR_TABLE_SLOTS = _lib.NEIGHBOUR_SCALE_BITS, _lib.NEIGHBOUR_TABLE_SLOTS
NEIGHBOUR_KINDS = {"cn": _lib.NEIGHBOUR_CN, "jaccard": _lib.NEIGHBOUR_JACCARD, "aa": _lib.NEIGHBOUR_AA, "ra": _lib.NEIGHBOUR_RA}
_ERRORS = ((_lib.NEIGHBOUR_ERR_COLUMN, "a column outside [0, n)"), (_lib.NEIGHBOUR_ERR_ORDER, "a row that is not ascending"),
           (_lib.NEIGHBOUR_ERR_QUERY, "a query index outside [0, n)"), (_lib.NEIGHBOUR_ERR_TABLE, "a full hash table"),
           (_lib.NEIGHBOUR_ERR_INDPTR, "a row pointer outside [0, nnz]"))

NeighbourScores = collections.namedtuple("NeighbourScores", [
    "common", "deg_i", "deg_j", "union", "cn", "jaccard", "aa", "ra", "pa", "aa_sum", "ra_sum"])
NeighbourScores.__doc__ = """per pair: common, deg_i, deg_j, union int32 [m]; cn int32 (= common); jaccard, aa, ra fp64;
pa int64; aa_sum, ra_sum int64, the fixed-point sums (aa = double(aa_sum) * 2^-32)."""
NeighbourTopK = collections.namedtuple("NeighbourTopK", ["index", "value", "common"])
NeighbourTopK.__doc__ = """index int32 [m, k] (-1: padding), value fp64 [m, k] (-inf at the padding), common int32 [m, k]."""

_last_routes = (0, 0)


def neighbour_last_routes():
    """(short rows, long rows) of this process's last ``neighbour_topk``: which route the rows took"""
    return _last_routes


def neighbour_weight_table(max_degree):
    """int64 [max_degree + 1, 2] on the host: column 0 rint(2^32 / log(d)) for d >= 2, column 1 rint(2^32 / d) for d >= 1,
    zero below (numpy fp64; the reference makes the same calls)"""
    d = np.arange(int(max_degree) + 1, dtype=np.float64)
    scale = np.float64(2.0) ** NEIGHBOUR_SCALE_BITS
    table = np.zeros((d.shape[0], 2), dtype=np.int64)
    table[2:, 0] = np.rint(scale / np.log(d[2:])).astype(np.int64)
    table[1:, 1] = np.rint(scale / d[1:]).astype(np.int64)
    return table


def _raise_status(who, status):
    host = status.cpu()                                    # the one read of the call
    bits = int(host[0])
    if bits:
        what = ", ".join(text for bit, text in _ERRORS if bits & bit)
        raise GaeHipError(f"{who}: the device reported error flags 0x{bits:x} ({what})")
    return host


def _symmetric_csr(graph, who):
    indptr, indices = graph.csr()
    t_indptr, t_indices = graph.csc()
    _gpu(indptr, f"{who}: graph")
    with _on_device(indptr.device):
        if not (torch.equal(indptr, t_indptr) and torch.equal(indices, t_indices)):
            raise GaeHipError(f"{who}: the graph is not symmetric (its CSR differs from the CSR of its transpose); "
                              "list every edge in both directions")
    return indptr.contiguous(), indices.contiguous()


def _degrees(indptr, indices, who):
    dev = indptr.device
    n = indptr.shape[0] - 1
    deg = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.zeros(_lib.NEIGHBOUR_STATUS_WORDS, dtype=torch.int64, device=dev)
    _lib.call("gae_neighbour_degrees", _ptr(indptr), _ptr(indices), n, indices.shape[0], _ptr(deg), _ptr(status), _stream())
    _raise_status(who, status)
    return deg


def neighbour_weights(graph):
    """``(deg, W)`` of a symmetric Graph on the GPU, for reuse across calls: deg int32 [n] (distinct non-self neighbours), W
    int64 [n, 2] (the Adamic-Adar and resource-allocation weight of every node, gathered from ``neighbour_weight_table``).  A
    column outside the graph or a row that is not ascending raises GaeHipError."""
    who = "neighbour_weights"
    with torch.no_grad():
        indptr, indices = _symmetric_csr(graph, who)
        with _on_device(indptr.device):
            deg = _degrees(indptr, indices, who)
            top = int(deg.max()) if deg.numel() else 0
            table = torch.from_numpy(neighbour_weight_table(top)).to(indptr.device)
            W = table.index_select(0, deg.long()).contiguous()
    return deg, W


def _weights_of(graph, weights, who):
    deg, W = neighbour_weights(graph) if weights is None else weights
    n = graph.csr()[0].shape[0] - 1
    if deg.dtype != torch.int32 or W.dtype != torch.int64 or tuple(deg.shape) != (n,) or tuple(W.shape) != (n, 2) \
            or not W.is_contiguous():
        raise GaeHipError(f"{who}: weights must be the (deg int32 [n], W int64 [n, 2]) pair of neighbour_weights")
    return deg, W


def neighbour_scores(graph, pairs, *, weights=None):
    """``NeighbourScores`` of the pairs int [2, m] (device tensor) on ``graph`` (a symmetric Graph on the GPU; duplicate edges
    and self-loops do not count).  ``weights``: the result of ``neighbour_weights(graph)``, to skip its two launches.  i == j
    is allowed (common = deg).  A pair outside [0, n), an asymmetric graph or a CPU tensor raises GaeHipError; there is no
    other route behind this function."""
    who = "neighbour_scores"
    pairs = _gpu(pairs, f"{who}: pairs")
    if pairs.dim() != 2 or pairs.shape[0] != 2 or pairs.dtype not in (torch.int32, torch.int64):
        raise GaeHipError(f"{who}: pairs must be an int32 / int64 [2, m] tensor, got {pairs.dtype} {tuple(pairs.shape)}")
    with torch.no_grad():
        deg, W = _weights_of(graph, weights, who)
        indptr, indices = (t.contiguous() for t in graph.csr())
        dev = indptr.device
        if weights is not None:
            _symmetric_csr(graph, who)
        if pairs.device != dev:
            raise GaeHipError(f"{who}: pairs are on {pairs.device}, the graph on {dev}")
        n, m = indptr.shape[0] - 1, pairs.shape[1]
        wide = pairs.long()
        if m and (int(wide.min()) < -2 ** 31 or int(wide.max()) >= 2 ** 31):
            raise GaeHipError(f"{who}: a pair index does not fit int32")
        pi, pj = wide[0].to(torch.int32).contiguous(), wide[1].to(torch.int32).contiguous()
        with _on_device(dev):
            common = torch.empty(m, dtype=torch.int32, device=dev)
            wsum = torch.empty(m, 2, dtype=torch.int64, device=dev)
            status = torch.zeros(_lib.NEIGHBOUR_STATUS_WORDS, dtype=torch.int64, device=dev)

            def launch():
                _lib.call("gae_neighbour_pairs", _ptr(indptr), _ptr(indices), n, indices.shape[0], _ptr(pi), _ptr(pj), m,
                          _ptr(W), 2, _ptr(common), _ptr(wsum), _ptr(status), _stream())
            _timed(("neighbour_pairs", n, m), launch)
            _raise_status(who, status)
            deg_i, deg_j = deg.index_select(0, pi.long()), deg.index_select(0, pj.long())
            union = deg_i + deg_j - common
            jaccard = torch.where(union > 0, common.double() / union.double(), torch.zeros((), dtype=torch.float64, device=dev))
            inv = 2.0 ** -NEIGHBOUR_SCALE_BITS
            aa_sum, ra_sum = wsum[:, 0].contiguous(), wsum[:, 1].contiguous()
            return NeighbourScores(common, deg_i, deg_j, union, common, jaccard, aa_sum.double() * inv, ra_sum.double() * inv,
                                   deg_i.long() * deg_j.long(), aa_sum, ra_sum)


def neighbour_topk(graph, k, kind="aa", *, rows=None, exclude_edges=True, table_slots=0, weights=None):
    """``NeighbourTopK``: for every query row (``rows`` int [m] device tensor, any order, repeats allowed; None: every node)
    the ``k`` (1..64) best candidates under ``kind`` ("cn", "jaccard", "aa", "ra").  Candidates of row i: every j != i with
    at least one common neighbour, minus the neighbours of i under ``exclude_edges``.  Order: larger value first (the integer
    count or fixed-point sum; the fp64 quotient for jaccard), then lower j.  Short rows pad with index -1, value -inf.
    ``table_slots`` (0: the default; a power of two in 64..2048) moves the bound between the hash-table route and the window
    route and never changes a bit of the result.  "pa" is not a local score and is refused."""
    global _last_routes
    who = "neighbour_topk"
    if kind not in NEIGHBOUR_KINDS:
        raise GaeHipError(f"{who}: kind = {kind!r}, not one of 'cn', 'jaccard', 'aa', 'ra' ('pa' is not a local score)")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.NEIGHBOUR_MAX_K:
        raise GaeHipError(f"{who}: k = {k!r} outside 1..{_lib.NEIGHBOUR_MAX_K}")
    if isinstance(table_slots, bool) or not isinstance(table_slots, int):
        raise GaeHipError(f"{who}: table_slots = {table_slots!r} must be an integer")
    with torch.no_grad():
        deg, W = _weights_of(graph, weights, who)
        indptr, indices = (t.contiguous() for t in graph.csr())
        dev = indptr.device
        if weights is not None:
            _symmetric_csr(graph, who)
        n = indptr.shape[0] - 1
        if rows is not None:
            rows = _gpu(rows, f"{who}: rows")
            if rows.dim() != 1 or rows.dtype not in (torch.int32, torch.int64) or rows.device != dev:
                raise GaeHipError(f"{who}: rows must be an int32 / int64 [m] tensor on the graph's device")
            if rows.numel() and (int(rows.min()) < -2 ** 31 or int(rows.max()) >= 2 ** 31):
                raise GaeHipError(f"{who}: a row index does not fit int32")
            rows = rows.to(torch.int32).contiguous()
        m = n if rows is None else rows.numel()
        code = NEIGHBOUR_KINDS[kind]
        col = {"aa": 0, "ra": 1}.get(kind)
        w_ptr = None if col is None else W.data_ptr() + 8 * col
        with _on_device(dev):
            index = torch.empty(m, k, dtype=torch.int32, device=dev)
            common = torch.empty(m, k, dtype=torch.int32, device=dev)
            wsum = torch.empty(m, k, dtype=torch.int64, device=dev)
            status = torch.zeros(_lib.NEIGHBOUR_STATUS_WORDS, dtype=torch.int64, device=dev)
            ws = torch.empty(_ws_bytes("gae_neighbour_topk_workspace_bytes", n, m), dtype=torch.uint8, device=dev)

            def launch():
                _lib.call("gae_neighbour_topk", _ptr(indptr), _ptr(indices), n, indices.shape[0], _ptr(rows), m, k, code,
                          w_ptr, 2, _ptr(deg), _lib.NEIGHBOUR_EXCLUDE_EDGES if exclude_edges else 0, table_slots,
                          _ptr(index), _ptr(common), _ptr(wsum), _ptr(status), _ptr(ws), ws.numel(), _stream())
            _timed(("neighbour_topk", n, m, k, kind), launch)
            host = _raise_status(who, status)
            _last_routes = (int(host[1]), int(host[2]))
            valid = index >= 0
            if kind == "cn":
                value = common.double()
            elif kind == "jaccard":
                src = torch.arange(n, device=dev) if rows is None else rows.long()
                deg_i = deg.index_select(0, src).unsqueeze(1).expand(m, k)
                deg_j = deg.index_select(0, index.clamp(min=0).long().reshape(-1)).reshape(m, k)
                union = deg_i + deg_j - common
                value = common.double() / union.clamp(min=1).double()
            else:
                value = wsum.double() * 2.0 ** -NEIGHBOUR_SCALE_BITS
            value = torch.where(valid, value, torch.full((), float("-inf"), dtype=torch.float64, device=dev))
            return NeighbourTopK(index, value, common)
