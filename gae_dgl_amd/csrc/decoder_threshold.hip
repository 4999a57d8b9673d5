// K22: the decoded graph without the N x N matrix (GAE.reconstruct, ops.decoder_threshold).
//
// A_hat = 1[sigmoid(z_i . z_j) >= p] of gae.py:69-72 as a CSR: for every row i the candidates c of decoder_pairs.h --
// window, self, known edges, score neither NaN nor -inf -- with s_ic >= threshold, columns ascending, and their
// scores.  Who is a candidate, how the columns are split over waves and which bits s_ic has: decoder_pairs.h, shared
// with K16 and K18 -- a listed score is the number gae_decoder_topk lists for that pair.
//
// Ordered compaction in three kinds of launches, none of which waits on another block:
//   count  one wave per (panel of 32 rows, column split) sweeps its tiles; a lane turns the 16 scores of its (row, lane
//          half) into the bits of the tile's columns that pass (passing()), and adds their number up.  The two halves
//          of a row meet in the wave; one int32 per (row, split) goes to the workspace.
//   scan   an exclusive int64 prefix sum over the (row, split) counts, row-major with the split minor: 1024 counts per
//          block, then one block over the block sums, then the sums added back -- ordinary launches.  Row i of row_ptr
//          is the offset of (i, 0), row_ptr[n] the total.
//   fill   the same sweep with the same passing().  Lane l and lane l + 32 exchange their bits (one __shfl_xor): the
//          row's 32-bit mask of the tile.  A pair goes to the (row, split) offset + what the row listed in earlier
//          tiles of this part (a per-lane running base) + the popcount of the mask below its column.
// No atomic decides a position: the layout is a function of the scores alone, so every schedule and every number of
// column splits writes the same bytes.  Every store is guarded by pos < capacity.
//
// passing().  A tile that lies inside the lane's window, does not hold the row itself (when self is excluded) and whose
// 16 scores add up to something above -inf (no NaN, no -inf among them) takes one compare per score; every other tile
// the masked form (LaneTile of decoder_pairs.h, K18's rule with one excluded column).  Only the columns that passed are
// looked up in the CSR row (row_holds), so a sparse decode pays almost nothing for GAE_TOPK_EXCLUDE_EDGES.
//
// Operand loads and the sweep are K18's (load_feats and sweep_tiles of decoder_pairs.h): row and feature clamped, tail
// features zeroed, the next tile's loads in flight while the current tile is multiplied and compacted.  Accumulators in
// VGPRs (-amdgpu-mfma-vgpr-form, _build.py): the epilogue reads each one.
//
// Measured (tools/decode_bench.py, profiles/r12_decoder_threshold.json; d = 16, one pair in a thousand listed, the whole
// call with its host sync): 0.51 ms at n = 19 717 (count 0.20, fill 0.27) and 43.4 ms at n = 200 000 for 4.2e7 pairs
// (count 18.2 ms -- K18's sweep --, fill 25.1 ms).
#include "decoder_pairs.h"

namespace {

using namespace gae::pairs;

constexpr int kScanThreads = 256;
constexpr int kScanItems = 4;
constexpr int kScanBlock = kScanThreads * kScanItems;      // (row, split) counts per block of the scan

struct ThresholdArgs : Common {
    float threshold;
    int32_t *count;               // [n][S]: passing pairs of (row, split)
    int64_t *offset;              // [n][S]: where the pairs of (row, split) start
    int64_t *block_sum;           // [nb + 1]: the scan's block sums, then their exclusive prefix and the total
    int64_t M, nb;                // n S, and its blocks of kScanBlock
    int64_t *row_ptr_out;
    int32_t *index_out;
    float *score_out;
    int64_t capacity;
};

template <int DH, bool ONE, bool FILL>
__device__ __forceinline__ void sweep(const ThresholdArgs &a)
{
    const int lane = threadIdx.x, col = lane & 31, h = lane >> 5;
    const int64_t panel = blockIdx.x / a.S;
    const int split = blockIdx.x % a.S;
    const int64_t row = panel * kRows + col;
    const bool row_in = row < a.n;
    const int i = row_in ? int(row) : 0;           // a row past n is clamped: it has no window and lists nothing

    // ---- the row: member window, CSR row
    int w0 = 0, w1 = 0;
    if (row_in) member_window(a, i, w0, w1);
    int e0 = 0, e1 = 0;
    if (row_in && a.indptr) { e0 = a.indptr[i]; e1 = a.indptr[i + 1]; }
    // ---- the wave's column part and this lane's columns in it
    int pb, pe, lo, hi;
    wave_part(w0, w1, a.S, split, pb, pe, lo, hi);
    pb = __builtin_amdgcn_readfirstlane(pb);       // the same in every lane: scalar loop control
    pe = __builtin_amdgcn_readfirstlane(pe);

    // ---- operands (decoder_pairs.h): the panel rows (B operand) stay in registers with one chunk
    const bool full = no_tail<DH>(a);
    float zr[DH];
    if constexpr (ONE) load_feats(zr, a.Z, a.ldz, i, 0, h, a.d, full);

    const float thr = a.threshold;
    const int xs = a.excl_self && row_in ? i : -1; // the column left out as "self" (-1: none)
    // the bits of the tile's columns (bit c: column c0 + c) among this lane's 16 that are listed (LaneTile,
    // decoder_pairs.h)
    auto passing = [&](const v16f &acc, int c0) -> unsigned {
        const LaneTile w(lo, hi, c0);
        if (w.empty()) return 0u;
        const int x_r = tile_rel(xs, c0);
        unsigned m = 0;                            // bits of lane half 0's columns; moved to this half's below
        if (w.all_candidates(acc, x_r)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) m |= acc[r] >= thr ? 1u << tile_col(0, r, 0) : 0u;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool ok = w.candidate(tile_col(0, r, h), acc[r], x_r) && acc[r] >= thr;
                m |= ok ? 1u << tile_col(0, r, 0) : 0u;
            }
        }
        m <<= 4 * h;
        if (a.indptr) {                            // known edges: only what passed is looked up
            for (unsigned rest = m; rest; rest &= rest - 1) {
                const int c = __ffs(int(rest)) - 1;
                if (row_holds(a.indices, e0, e1, c0 + c)) m &= ~(1u << c);
            }
        }
        return m;
    };

    int count = 0;
    int64_t base = 0;                              // fill: where the row's next listed pair of this part goes
    if constexpr (FILL) base = row_in ? a.offset[row * a.S + split] : 0;
    sweep_tiles<DH, ONE>(a, zr, i, col, h, full, pb, pe, [&](const v16f &acc, int c0) {
        const unsigned m = passing(acc, c0);
        if constexpr (FILL) {
            const unsigned both = m | unsigned(__shfl_xor(int(m), 32, 64));      // the row's 32 columns of the tile
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = tile_col(0, r, h);
                if ((m >> c) & 1u) {
                    const int64_t pos = base + __popc(both & ((1u << c) - 1u));
                    if (pos < a.capacity) {
                        a.index_out[pos] = c0 + c;
                        a.score_out[pos] = acc[r];
                    }
                }
            }
            base += __popc(both);
        } else {
            count += __popc(m);
        }
    });

    if constexpr (!FILL) {
        count += __shfl_down(count, 32, 64);       // the two lane halves of each row; lane half 0 writes
        if (h == 0 && row_in) a.count[row * a.S + split] = count;
    }
}

template <int DH, bool ONE>
__global__ __launch_bounds__(64) void threshold_count_kernel(const ThresholdArgs a) { sweep<DH, ONE, false>(a); }

template <int DH, bool ONE>
__global__ __launch_bounds__(64) void threshold_fill_kernel(const ThresholdArgs a) { sweep<DH, ONE, true>(a); }

// ---- the scan: three ordinary launches
// exclusive prefix of v over the kScanThreads threads of a block (thread order); total = the block's sum.  lds: [4]
__device__ __forceinline__ int64_t block_excl_scan(int64_t v, int64_t *lds, int64_t &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int64_t o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    __syncthreads();                               // the previous call's readers are done with lds
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int64_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / 64; ++w) {
        const int64_t t = lds[w];
        before += w < wave ? t : 0;
        total += t;
    }
    return before + incl - v;
}

// block b: offset[e] = the exclusive prefix of count inside the block, block_sum[b] = the block's sum
__global__ __launch_bounds__(kScanThreads) void threshold_scan_blocks_kernel(const ThresholdArgs a)
{
    __shared__ int64_t lds[kScanThreads / 64];
    const int64_t e0 = int64_t(blockIdx.x) * kScanBlock + int64_t(threadIdx.x) * kScanItems;
    int32_t c[kScanItems];
    int64_t mine = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        c[k] = e0 + k < a.M ? a.count[e0 + k] : 0;
        mine += c[k];
    }
    int64_t total;
    int64_t at = block_excl_scan(mine, lds, total);
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (e0 + k < a.M) a.offset[e0 + k] = at;
        at += c[k];
    }
    if (threadIdx.x == 0) a.block_sum[blockIdx.x] = total;
}

// one block: block_sum[0 .. nb) becomes its exclusive prefix, block_sum[nb] the total
__global__ __launch_bounds__(kScanThreads) void threshold_scan_sums_kernel(const ThresholdArgs a)
{
    __shared__ int64_t lds[kScanThreads / 64];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < a.nb; b0 += kScanThreads) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t v = b < a.nb ? a.block_sum[b] : 0;
        int64_t total;
        const int64_t at = block_excl_scan(v, lds, total);
        if (b < a.nb) a.block_sum[b] = carry + at;
        carry += total;
    }
    if (threadIdx.x == 0) a.block_sum[a.nb] = carry;
}

// offset[e] += the prefix of its block; row i of row_ptr_out = the offset of (i, 0), row n = the total
__global__ __launch_bounds__(kScanThreads) void threshold_scan_add_kernel(const ThresholdArgs a)
{
    const int64_t e0 = int64_t(blockIdx.x) * kScanBlock + int64_t(threadIdx.x) * kScanItems;
    const int64_t before = blockIdx.x < a.nb ? a.block_sum[blockIdx.x] : 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int64_t e = e0 + k;
        if (e < a.M) {
            const int64_t v = a.offset[e] + before;
            a.offset[e] = v;
            if (e % a.S == 0) a.row_ptr_out[e / a.S] = v;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) a.row_ptr_out[a.n] = a.block_sum[a.nb];
}

// ---- host side: what both entry points derive from the selection arguments
struct Layout {
    int S;
    int64_t panels, M, nb, need;
    int64_t *offset, *block_sum; int32_t *count;   // the workspace regions (NULL for the size query)
};

int plan(const char *fn, const Request &r, float threshold, int64_t splits_arg, void *ws, Layout &L)
{
    GAE_REQUIRE(threshold == threshold, GAE_E_RANGE, "%s: threshold is NaN", fn);
    GAE_REQUIRE(splits_arg >= 0 && splits_arg <= kMaxSplits, GAE_E_RANGE, "%s: splits = %lld outside 0..16", fn,
                (long long)splits_arg);
    if (const int rc = check_sizes(fn, r)) return rc;
    L.panels = (r.n + kRows - 1) / kRows;
    L.S = splits(L.panels, r.n, r.node_ptr, r.max_graph_nodes, int(splits_arg));
    L.M = r.n * L.S;
    L.nb = (L.M + kScanBlock - 1) / kScanBlock;
    gae::Carver c(ws);                             // THE layout: behind 256 bytes, three regions packed at 8-byte steps
    c.raw<char>(256);
    L.offset = c.raw<int64_t>(8 * L.M);
    L.block_sum = c.raw<int64_t>(8 * (L.nb + 1));
    L.count = c.raw<int32_t>(4 * L.M);
    c.round();
    L.need = c.bytes();
    return GAE_OK;
}

void fill_args(ThresholdArgs &a, const Request &r, const Layout &L, float threshold)
{
    fill(a, r, L.S);
    a.threshold = threshold;
    a.offset = L.offset; a.block_sum = L.block_sum; a.count = L.count;
    a.M = L.M; a.nb = L.nb;
    a.row_ptr_out = nullptr; a.index_out = nullptr; a.score_out = nullptr; a.capacity = 0;
}

} // namespace

extern "C" int gae_decoder_threshold_count(const float *Z, int64_t ldz, int64_t n, int64_t d, float threshold,
                                           const int64_t *node_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                                           const int32_t *indptr, const int32_t *indices, int flags, int64_t splits,
                                           int64_t *row_ptr_out, void *workspace, int64_t *workspace_bytes,
                                           void *stream)
{
    const char *fn = "gae_decoder_threshold_count";
    const Request r{Z, ldz, n, d, node_ptr, n_graphs, max_graph_nodes, indptr, indices, flags, workspace_bytes};
    Layout L;
    if (const int rc = plan(fn, r, threshold, splits, workspace, L)) return rc;
    if (!workspace) {                               // size query: no device work
        *workspace_bytes = L.need;
        return GAE_OK;
    }
    GAE_REQUIRE(row_ptr_out, GAE_E_NULL, "%s: row_ptr_out is NULL", fn);
    if (const int rc = check_arrays(fn, r, L.need)) return rc;
    ThresholdArgs a;
    fill_args(a, r, L, threshold);
    a.row_ptr_out = row_ptr_out;
    hipStream_t st = gae::as_stream(stream);
    if (n > 0) {
        dispatch(d, [&](auto dh, auto one) {
            hipLaunchKernelGGL((threshold_count_kernel<dh, one>), dim3(unsigned(L.panels * L.S)), dim3(64), 0, st, a);
        });
        GAE_CHECK_LAUNCH("threshold_count_kernel");
        hipLaunchKernelGGL(threshold_scan_blocks_kernel, dim3(unsigned(L.nb)), dim3(kScanThreads), 0, st, a);
        GAE_CHECK_LAUNCH("threshold_scan_blocks_kernel");
    }
    hipLaunchKernelGGL(threshold_scan_sums_kernel, dim3(1), dim3(kScanThreads), 0, st, a);
    GAE_CHECK_LAUNCH("threshold_scan_sums_kernel");
    hipLaunchKernelGGL(threshold_scan_add_kernel, dim3(unsigned(L.nb > 0 ? L.nb : 1)), dim3(kScanThreads), 0, st, a);
    GAE_CHECK_LAUNCH("threshold_scan_add_kernel");
    return GAE_OK;
}

extern "C" int gae_decoder_threshold_fill(const float *Z, int64_t ldz, int64_t n, int64_t d, float threshold,
                                          const int64_t *node_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                                          const int32_t *indptr, const int32_t *indices, int flags, int64_t splits,
                                          const int64_t *row_ptr, int32_t *index_out, float *score_out,
                                          int64_t capacity, void *workspace, int64_t *workspace_bytes, void *stream)
{
    const char *fn = "gae_decoder_threshold_fill";
    const Request r{Z, ldz, n, d, node_ptr, n_graphs, max_graph_nodes, indptr, indices, flags, workspace_bytes};
    Layout L;
    if (const int rc = plan(fn, r, threshold, splits, workspace, L)) return rc;
    if (!workspace) {                               // size query: no device work
        *workspace_bytes = L.need;
        return GAE_OK;
    }
    GAE_REQUIRE(capacity >= 0, GAE_E_SIZE, "%s: negative capacity = %lld", fn, (long long)capacity);
    GAE_REQUIRE(row_ptr, GAE_E_NULL, "%s: row_ptr is NULL", fn);
    GAE_REQUIRE(capacity == 0 || (index_out && score_out), GAE_E_NULL, "%s: index_out / score_out is NULL", fn);
    if (const int rc = check_arrays(fn, r, L.need)) return rc;
    if (n == 0 || capacity == 0) return GAE_OK;
    ThresholdArgs a;
    fill_args(a, r, L, threshold);
    a.index_out = index_out; a.score_out = score_out; a.capacity = capacity;
    hipStream_t st = gae::as_stream(stream);
    dispatch(d, [&](auto dh, auto one) {
        hipLaunchKernelGGL((threshold_fill_kernel<dh, one>), dim3(unsigned(L.panels * L.S)), dim3(64), 0, st, a);
    });
    GAE_CHECK_LAUNCH("threshold_fill_kernel");
    return GAE_OK;
}
