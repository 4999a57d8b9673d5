// K18: filtered link ranking without the N x N matrix (GAE.rank_links, ops.decoder_rank).
//
// For query q = (i, j) = (src[q], dst[q]) and t = s_ij = z_i . z_j: how many candidates c of row i, the target left out,
// score above t and how many score exactly t -- the rank of j among all candidates of i (MRR, Hits@K, mean rank, the
// exact all-negatives AUC; metrics.rank_metrics).  Who is a candidate, how the columns are split over waves and which
// bits s_ic has: decoder_pairs.h, shared with K16 -- s_ic is the number gae_decoder_topk lists for that pair.
//
// Products.  Panel row r holds z_{src[q0 + r]} (gathered); the tiles of Z are the other operand.
// The threshold t comes out of the same instruction: one extra tile whose A operand is the gathered dst rows; the lane
// that owns the diagonal element (row r against column r) hands it to the other half of its row.  No score is computed
// by a second route, so "s_ic == t" is an equality of bits of one and the same chain.
//
// Counting.  Each lane keeps three int32 counts of its (query, lane half): scores above t, scores at or above t, valid
// scores.  A tile that lies inside the lane's window, holds neither i (when self is excluded) nor j, and whose 16
// scores add up to something above -inf (no NaN, no -inf among them) takes the fast path: two compares and two adds
// per score plus the sum.  Every other tile takes the masked path (window, self, target, validity per column).  The
// rule is LaneTile of decoder_pairs.h, shared with K22.
//
// Known edges.  The sweep counts them like any column; a second sweep takes them out again.  The CSR rows of the
// panel's 32 sources are laid end to end, 32 entries per tile: the A operand gathers those columns, the same MFMA
// gives their scores, and a lane looks only at the slots of its own row.  A repeated entry counts once: the lane
// that gathers entry e tells whether e is the first occurrence of its column -- from its left neighbour when the
// row is sorted (checked once per row), by a scan of the entries before it otherwise (quadratic in the degree of an
// UNSORTED row only).  Tiles of the second sweep are dealt round-robin to the column splits.
//
// Output.  The two lane halves of a query add up in the wave.  With one column split the wave writes the result; with
// S > 1 every (panel, split) wave stores its three partial counts in the workspace and a second launch adds the S
// parts: integers, so every schedule gives the same bits.
//
// Measured (tools/rank_bench.py, profiles/r09_decoder_rank.json; d = 16, m = n, a 5-regular graph excluded): 0.25 ms at
// n = 19 717 and 19.2 ms at n = 200 000 (66 Tflop/s of fp32 MFMA, 42 % of peak) -- 0.27 x and 0.52 x the time of
// gae_decoder_topk(k = 10) on the same Z.  What buys that: operand loads without branches (row and feature clamped, two
// 16-byte loads per tile at d = 16) and the next tile's loads issued before the current tile is counted (load_feats and
// sweep_tiles of decoder_pairs.h, shared with K22).  118 VGPRs at
// d <= 16 (4 waves per SIMD), accumulators in VGPRs (-amdgpu-mfma-vgpr-form, _build.py): the epilogue reads each one.
#include "decoder_pairs.h"

namespace {

using namespace gae::pairs;

struct RankArgs : Common {
    int m;
    const int64_t *src, *dst;
    float *score_out;
    int64_t *greater_out, *equal_out, *cand_out;
    int32_t *part;                // [S][m][3] (S > 1): above, at-or-above, valid
};

__device__ __forceinline__ void write_result(const RankArgs &a, int64_t q, bool ok, float t, int gt, int ge, int valid)
{
    int64_t g = -1, e = -1, c = -1;
    if (ok) {
        const bool tnan = t != t;                 // a NaN target ranks last
        g = tnan ? valid : gt;
        e = tnan ? 0 : ge - gt;
        c = valid;
    }
    a.score_out[q] = ok ? t : __builtin_nanf("");
    a.greater_out[q] = g;
    a.equal_out[q] = e;
    a.cand_out[q] = c;
}

template <int DH, bool ONE>
__global__ __launch_bounds__(64) void rank_kernel(const RankArgs a)
{
    __shared__ int64_t s_pref[kRows + 1];          // CSR rows of the panel laid end to end: first slot of row r
    __shared__ int s_e0[kRows];
    __shared__ int s_sorted[kRows];
    __shared__ int s_col[kTile];                   // second sweep: the column each slot gathered, -1 = not counted
    const int lane = threadIdx.x, col = lane & 31, h = lane >> 5;
    const int panel = blockIdx.x / a.S, split = blockIdx.x % a.S;
    const int64_t q = int64_t(panel) * kRows + col;
    const bool q_in = q < a.m;
    const int64_t si = q_in ? a.src[q] : -1, sj = q_in ? a.dst[q] : -1;
    const bool ok = si >= 0 && si < a.n && sj >= 0 && sj < a.n;      // an index outside [0, n) loads nothing
    const int i = ok ? int(si) : 0, j = ok ? int(sj) : 0;

    // ---- the query's row: member window, CSR row
    int w0 = 0, w1 = 0;
    if (ok) member_window(a, i, w0, w1);
    int e0 = 0, e1 = 0;
    if (ok && a.indptr) { e0 = a.indptr[i]; e1 = a.indptr[i + 1]; }
    // ---- the wave's column part and this lane's columns in it
    int pb, pe, lo, hi;
    wave_part(w0, w1, a.S, split, pb, pe, lo, hi);
    pb = __builtin_amdgcn_readfirstlane(pb);       // the same in every lane: scalar loop control
    pe = __builtin_amdgcn_readfirstlane(pe);

    // ---- operands (decoder_pairs.h): the panel rows (B operand) stay in registers when one chunk holds all of d
    const bool full = no_tail<DH>(a);
    float zr[DH];
    if constexpr (ONE) load_feats(zr, a.Z, a.ldz, i, 0, h, a.d, full);
    // one tile: rows of Z picked by `row` (in [0, n)) against the panel
    auto tile = [&](int64_t row) { return tile_product<DH, ONE>(a, zr, i, row, h, full); };

    // ---- the threshold: the diagonal of (gathered dst rows) x (panel), row `col` against column `col` of this tile
    float t;
    {
        const v16f acc = tile(j);
        int owner, dr;
        tile_owner(col, col, owner, dr);
        float dv = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) dv = r == dr ? acc[r] : dv;
        t = __shfl(dv, owner, 64);
    }

    int gt = 0, ge = 0, valid = 0;
    const int xs = a.excl_self ? i : -1;           // the column left out as "self" (-1: none)
    // counts of one tile at c0: the target is left out like self (LaneTile, decoder_pairs.h)
    sweep_tiles<DH, ONE>(a, zr, i, col, h, full, pb, pe, [&](const v16f &acc, int c0) {
        const LaneTile w(lo, hi, c0);
        if (w.empty()) return;
        const int j_r = tile_rel(j, c0), x_r = tile_rel(xs, c0);
        if (w.all_candidates(acc, j_r, x_r)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                gt += acc[r] > t ? 1 : 0;
                ge += acc[r] >= t ? 1 : 0;
            }
            valid += 16;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool cand = w.candidate(tile_col(0, r, h), acc[r], j_r, x_r);
                gt += (cand && acc[r] > t) ? 1 : 0;
                ge += (cand && acc[r] >= t) ? 1 : 0;
                valid += cand ? 1 : 0;
            }
        }
    });

    // ---- known edges: take the distinct neighbours the sweep counted out again
    if (a.indptr) {
        const int deg = e1 > e0 ? e1 - e0 : 0;
        int64_t incl = deg;                        // inclusive prefix over the 32 rows (both halves compute the same)
        for (int off = 1; off < 32; off <<= 1) {
            const int64_t o = __shfl_up(incl, off, 32);
            if (col >= off) incl += o;
        }
        const int64_t pref = incl - deg;
        const int64_t total = __shfl(incl, 31, 64);
        // is the row sorted (non-decreasing)?  each half checks half of it
        int sorted = 1;
        {
            const int xb = e0 + 1, xe = e1 > e0 ? e1 : e0 + 1;  // pairs (x - 1, x), x in [xb, xe)
            const int xm = xb + (xe - xb) / 2;
            for (int x = h == 0 ? xb : xm; x < (h == 0 ? xm : xe); ++x)
                sorted &= a.indices[x - 1] <= a.indices[x] ? 1 : 0;
            sorted &= __shfl_xor(sorted, 32, 64);
        }
        if (h == 0) {
            s_pref[col] = pref;
            s_e0[col] = e0;
            s_sorted[col] = sorted;
            if (col == 31) s_pref[32] = total;
        }
        __syncthreads();
        const int64_t ntiles = (total + kTile - 1) / kTile;
        for (int64_t tix = split; tix < ntiles; tix += a.S) {
            // slot p of the concatenation: owner row, entry, column; is it the first occurrence in its row?
            const int64_t p = tix * kTile + col;
            int c = -1;
            if (p < total) {
                int l = 0, u = kRows;              // last row o with s_pref[o] <= p (it has an entry: s_pref[o + 1] > p)
                while (u - l > 1) { const int mid = (l + u) >> 1; if (s_pref[mid] <= p) l = mid; else u = mid; }
                const int b = s_e0[l];
                const int e = b + int(p - s_pref[l]);
                const int v = a.indices[e];
                const bool first = s_sorted[l] ? e == b || a.indices[e - 1] != v : !row_holds(a.indices, b, e, v);
                if (first && v >= 0 && v < a.n) c = v;             // a bad CSR entry never reads outside Z
            }
            __syncthreads();                       // the previous tile's readers are done with s_col
            if (h == 0) s_col[col] = c;
            __syncthreads();
            const v16f acc = tile(c >= 0 ? c : 0);
            const int64_t base = tix * kTile;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int s = tile_col(0, r, h);
                const int64_t ps = base + s;
                const int cs = s_col[s];
                // mine, and counted by the sweep: inside the row's whole window, neither the target nor self, valid
                const bool cand = ps >= pref && ps < pref + deg && cs >= w0 && cs < w1 && cs != j && cs != xs &&
                                  acc[r] > -INFINITY;
                gt -= (cand && acc[r] > t) ? 1 : 0;
                ge -= (cand && acc[r] >= t) ? 1 : 0;
                valid -= cand ? 1 : 0;
            }
        }
    }

    // ---- the two lane halves of each query; lane half 0 writes
    gt += __shfl_down(gt, 32, 64);
    ge += __shfl_down(ge, 32, 64);
    valid += __shfl_down(valid, 32, 64);
    if (h == 0 && q_in) {
        if (a.S == 1) {
            write_result(a, q, ok, t, gt, ge, valid);
        } else {
            int32_t *p = a.part + (int64_t(split) * a.m + q) * 3;
            p[0] = gt; p[1] = ge; p[2] = valid;
            if (split == 0) a.score_out[q] = t;
        }
    }
}

// one thread per query: the S partial counts added up (a part may be negative: the second sweep of one split takes
// out what the first sweep of another counted).  S = 0 (n = 0: no row of Z exists) only marks every query invalid.
__global__ __launch_bounds__(256) void rank_combine_kernel(const RankArgs a)
{
    const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (q >= a.m) return;
    const int64_t si = a.src[q], sj = a.dst[q];
    const bool ok = si >= 0 && si < a.n && sj >= 0 && sj < a.n;
    int gt = 0, ge = 0, valid = 0;
    for (int s = 0; s < a.S; ++s) {
        const int32_t *p = a.part + (int64_t(s) * a.m + q) * 3;
        gt += p[0]; ge += p[1]; valid += p[2];
    }
    write_result(a, q, ok, ok ? a.score_out[q] : 0.f, gt, ge, valid);
}

int64_t need_bytes(int64_t m, int S) { return S > 1 ? int64_t(S) * m * 12 + 256 : 256; }

} // namespace

namespace gae {
Knob g_rank_splits{0};       // "rank_splits": column splits per query panel, 0 = auto (tests force 1 or more)
} // namespace gae

extern "C" int gae_decoder_rank(const float *Z, int64_t ldz, int64_t n, int64_t d, const int64_t *src,
                                const int64_t *dst, int64_t m, const int64_t *node_ptr, int64_t n_graphs,
                                int64_t max_graph_nodes, const int32_t *indptr, const int32_t *indices, int flags,
                                float *score_out, int64_t *greater_out, int64_t *equal_out, int64_t *candidates_out,
                                void *workspace, int64_t *workspace_bytes, void *stream)
{
    const char *fn = "gae_decoder_rank";
    const Request r{Z, ldz, n, d, node_ptr, n_graphs, max_graph_nodes, indptr, indices, flags, workspace_bytes};
    GAE_REQUIRE(n >= 0 && m >= 0, GAE_E_SIZE, "%s: negative n = %lld or m = %lld", fn, (long long)n, (long long)m);
    GAE_REQUIRE(m < (int64_t(1) << 31), GAE_E_SIZE, "%s: m = %lld queries, 2^31 - 1 at most", fn, (long long)m);
    if (const int rc = check_sizes(fn, r)) return rc;
    const int64_t panels = (m + kRows - 1) / kRows;
    const int S = splits(panels, n, node_ptr, max_graph_nodes, gae::g_rank_splits);
    const int64_t need = need_bytes(m, S);
    if (!workspace) {                               // size query: no device work
        *workspace_bytes = need;
        return GAE_OK;
    }
    GAE_REQUIRE(m == 0 || (src && dst), GAE_E_NULL, "%s: src / dst is NULL", fn);
    GAE_REQUIRE(m == 0 || (score_out && greater_out && equal_out && candidates_out), GAE_E_NULL,
                "%s: score_out / greater_out / equal_out / candidates_out is NULL", fn);
    if (const int rc = check_arrays(fn, r, need)) return rc;
    if (m == 0) return GAE_OK;
    RankArgs a;
    fill(a, r, S);
    a.m = int(m); a.src = src; a.dst = dst;
    a.score_out = score_out; a.greater_out = greater_out; a.equal_out = equal_out; a.cand_out = candidates_out;
    a.part = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + 256);
    hipStream_t st = gae::as_stream(stream);
    if (n == 0) {
        a.S = 0;
        hipLaunchKernelGGL(rank_combine_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, st, a);
        GAE_CHECK_LAUNCH("rank_combine_kernel");
        return GAE_OK;
    }
    dispatch(d, [&](auto dh, auto one) {
        hipLaunchKernelGGL((rank_kernel<dh, one>), dim3(unsigned(panels * S)), dim3(64), 0, st, a);
    });
    GAE_CHECK_LAUNCH("rank_kernel");
    if (S > 1) {
        hipLaunchKernelGGL(rank_combine_kernel, dim3(unsigned((m + 255) / 256)), dim3(256), 0, st, a);
        GAE_CHECK_LAUNCH("rank_combine_kernel");
    }
    return GAE_OK;
}
