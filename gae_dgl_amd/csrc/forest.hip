// K26: a histogram-based regression forest on frozen features (ops.forest, GAE.forest_graphs, embed --forest).
//
// The contract -- binning, fixed-point targets, the Philox bootstrap and feature subsets, the score and its order of
// operations, the tie rules, node numbering, values, prediction, the status block -- is the K26 comment of
// include/gae_hip_experimental.h.  Every accumulated quantity is an integer (bin codes, int64 fixed-point targets, integer
// counts and sums), so integer atomics in LDS and in global memory are exact and free of order: no float atomics, the
// same bits run to run whatever the launch split.  This file is built with -ffp-contract=off (_build.py): the fp64 score
// and the node values are plain IEEE operations that numpy restates one to one (tests/forest_ref.py).
//
// LAYOUTS
//   codes     uint8 [n_used][d], row-major by LISTED row: the histogram kernel's consecutive threads read consecutive
//             features of one sample, d contiguous bytes per gathered row (12 MB for 249 455 x 48: L2-resident)
//   yq        int64 [n_used][t] fixed-point targets (workspace)
//   pos       int32 [T][n_boot], two buffers: each tree's samples (listed-row ids), kept partitioned by node after every
//             level, so a node is the contiguous segment [seg_start, seg_start + count)
//
// LAUNCHES of gae_forest_fit: fill (node tables), quantise (yq), bootstrap (pos, in-bag marks, root sums by int64 atomics),
// root (node 0 of every tree, the level-0 work lists); then per level, all trees at once:
//   hist      one block per (work item's chunk of <= GAE_FOREST_SPLIT_ROWS rows, feature tile): count and sum cells of
//             the tile in LDS by integer atomics.  A node that is one chunk scans its cells in the same block and emits
//             the tile's best candidate; a longer node adds its cells to a global slot (integer atomics) instead
//   scan      (only when some node is longer than a chunk) one block per (long node, feature tile): the merged cells
//             from the slot, the same scan
//   decide    one block per tree: the best candidate over the tiles, the split test against the parent's score, the
//             children's numbers from a block scan over the level's nodes in ascending id, the node records
//   partition one block per chunk: the segment of a node that split is partitioned into the other pos buffer; a chunk
//             reserves its ranges with two integer cursors per node (the order inside a segment is not part of any result)
//   emit      one block per tree: the next level's work items, chunk list and long-node slots, and the 32-byte level
//             status the host reads once per level (it sizes the next grids and stops the loop early)
// The node x feature x bin histogram never reaches HBM except the merged cells of nodes longer than one chunk.
// The bodies of hist, scan and partition and the tree walk of predict are the level pass of forest_cells.h, which K30
// (boost.hip) runs too; what is the forest's own there is its lists (node_of) and the Targets and Variance policies.
#include <float.h>

#include "common.h"
#include "forest_cells.h"

namespace {

using gae::cdiv;
using gae::up256;

constexpr int kMaxD = 256, kMaxT = 8, kMaxTrees = 1024, kMaxDepth = 16, kMaxBins = 256;
constexpr int kSplitRows = gae::cells::kSplitRows;
constexpr int kThreads = gae::cells::kThreads, kWaves = gae::cells::kWaves;
constexpr int kWalkSteps = 64;             // a walk longer than this is a broken node table, not a tree

using gae::cells::block_scan;
using gae::cells::Chunk;
using gae::cells::chunks_of;
using gae::cells::flag;
using gae::cells::i64;
using gae::cells::take_halves;
using gae::cells::u64;

__device__ __forceinline__ void count_nonfinite(gae_forest_status *st, int64_t v)
{
    atomicAdd(reinterpret_cast<u64 *>(&st->nonfinite), static_cast<u64>(v));
}

struct Item { int tree, node, slot, pad; };                // slot >= 0: a node longer than one chunk, its global cells
struct TreeInfo { int item_lo, item_n, base, n_new, tot_work, tot_chunks, tot_long, pad; };
struct Level { int64_t n_items, n_chunks, n_long, pad; };

struct FitArgs : gae::cells::Frame {                      // (the level pass's own arrays are the Frame's)
    const float *edges;
    const float *Y;
    const int32_t *rows;
    int64_t ldy;
    int n, t, T, n_boot, max_depth, bootstrap, M, level;
    float pivot[kMaxT];
    double up[kMaxT], inv[kMaxT], scale[kMaxT];            // 2^e, 2^-e, 4^-e
    // outputs
    int32_t *n_nodes;
    float *threshold;
    double *value, *gain;
    uint8_t *inbag;
    // workspace
    i64 *yq, *node_sum;
    int32_t *split_cur, *split_next;
    Item *items_cur, *items_next;
    Chunk *chunks_cur, *chunks_next;
    TreeInfo *info;
    Level *lvl;
};

// ------------------------------------------------------------------------------------------------------ set-up
__global__ __launch_bounds__(kThreads) void forest_fill_kernel(const FitArgs a)
{
    const int64_t total = int64_t(a.T) * a.M;
    for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < total; i += int64_t(gridDim.x) * kThreads) {
        a.feature[i] = -1; a.bin[i] = -1; a.left[i] = -1; a.count[i] = 0;
        a.threshold[i] = 0.f; a.gain[i] = 0.0;
        for (int j = 0; j < a.t; ++j) a.value[i * a.t + j] = 0.0;
    }
}

__global__ __launch_bounds__(kThreads) void forest_quant_kernel(const FitArgs a)
{
    const int64_t e = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (e >= int64_t(a.n_used) * a.t) return;
    const int i = int(e / a.t), j = int(e % a.t);
    const int row = a.rows ? a.rows[i] : i;
    i64 q = 0;
    if (unsigned(row) >= unsigned(a.n)) {
        flag(a.status, GAE_FOREST_ERR_ROW_ID);
    } else {
        const float v = a.Y[int64_t(row) * a.ldy + j];
        if (!(fabsf(v) <= FLT_MAX)) count_nonfinite(a.status, 1);
        else q = llrint((double(v) - double(a.pivot[j])) * a.up[j]);
    }
    a.yq[e] = q;
}

// grid (ceil(n_boot / 256), T)
__global__ __launch_bounds__(kThreads) void forest_boot_kernel(const FitArgs a)
{
    __shared__ i64 part[kWaves][kMaxT];
    const int tree = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t j = int64_t(blockIdx.x) * kThreads + tid;
    const bool on = j < a.n_boot;
    int s = 0;
    if (on) {
        if (a.bootstrap) {
            uint32_t c[4];
            gae::philox4x32_10(uint64_t(j) >> 2, uint64_t(tree), a.key, c);
            s = int((uint64_t(c[j & 3]) * uint64_t(a.n_used)) >> 32);
            if (a.inbag) a.inbag[int64_t(tree) * a.n_used + s] = 1;
        } else {
            s = int(j);
        }
        a.pos_in[int64_t(tree) * a.n_boot + j] = s;
    }
    for (int q = 0; q < a.t; ++q) {
        i64 v = on ? a.yq[int64_t(s) * a.t + q] : 0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) part[wave][q] = v;
    }
    __syncthreads();
    if (tid < a.t) {
        i64 v = 0;
        for (int w = 0; w < kWaves; ++w) v += part[w][tid];
        atomicAdd(reinterpret_cast<u64 *>(&a.node_sum[int64_t(tree) * a.M * a.t + tid]), static_cast<u64>(v));
    }
}

__device__ __forceinline__ void write_value(const FitArgs &a, int64_t node_at, int count)
{
    for (int j = 0; j < a.t; ++j)
        a.value[node_at * a.t + j] = double(a.pivot[j]) + (double(a.node_sum[node_at * a.t + j]) / double(count)) * a.inv[j];
}

// one thread per tree: node 0 and the level-0 lists (the level status of level 0 is the host's)
__global__ __launch_bounds__(kThreads) void forest_root_kernel(const FitArgs a, int offered)
{
    const int tree = blockIdx.x * kThreads + threadIdx.x;
    if (tree >= a.T) return;
    const int64_t at = int64_t(tree) * a.M;
    a.count[at] = a.n_boot;
    a.seg_start[at] = 0;
    a.n_nodes[tree] = 1;
    write_value(a, at, a.n_boot);
    TreeInfo ti = {tree, offered ? 1 : 0, 1, 0, 0, 0, 0, 0};
    a.info[tree] = ti;
    if (!offered) return;
    const int nch = chunks_of(a.n_boot);
    const bool is_long = a.n_boot > kSplitRows;
    a.items_cur[tree] = Item{tree, 0, is_long ? tree : -1, 0};
    a.curs[tree] = make_int2(0, 0);
    if (is_long) a.split_cur[tree] = tree;
    for (int c = 0; c < nch; ++c) a.chunks_cur[int64_t(tree) * nch + c] = Chunk{tree, c};
}

// ------------------------------------------------------------------------------------------------------ a level
using gae::cells::Lds;
using gae::cells::Node;

// work item `item` of the level: its node as the level pass sees it
__device__ __forceinline__ Node node_of(const FitArgs &a, int item)
{
    const Item it = a.items_cur[item];
    return Node{int64_t(it.tree) * a.M + it.node, int64_t(it.tree) * a.n_boot, item, it.slot, it.node,
                (uint64_t(1) << 32) + uint64_t(it.tree)};
}

// a cell holds t sums: the fixed-point targets of the listed rows
struct Targets {
    const FitArgs &a;
    __device__ int words() const { return a.t; }
    __device__ i64 word(int s, int j) const { return a.yq[int64_t(s) * a.t + j]; }
};

// the score of a split of node `at`: the sum over the targets of S_l^2 / n_l + S_r^2 / n_r, each in its own scale
struct Variance {
    const FitArgs &a;
    int64_t at;
    __device__ int words() const { return a.t; }
    __device__ double score(const Lds &h, int idx, int nl, int nr) const
    {
        const int t = a.t;
        double score = 0.0;
        for (int j = 0; j < t; ++j) {
            const i64 sl = h.sum[int64_t(idx) * t + j], sr = a.node_sum[at * t + j] - sl;
            const double dl = double(sl), dr = double(sr);
            const double term = (dl * dl / double(nl) + dr * dr / double(nr)) * a.scale[j];
            score = score + term;
        }
        return score;
    }
};

// grid n_chunks . nft: block b is tile b % nft of chunk b / nft
__global__ __launch_bounds__(kThreads) void forest_hist_kernel(const FitArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Lds h = gae::cells::carve(lds, a.ft, a.bins, a.t);
    const int tile = blockIdx.x % a.nft;
    const Chunk ch = a.chunks_cur[blockIdx.x / a.nft];
    const Node nd = node_of(a, ch.item);
    if (gae::cells::fill_tile(a, h, Targets{a}, nd, ch, tile)) return;     // a node of several chunks: scanned later
    gae::cells::scan_tile(a, h, Variance{a, nd.at}, nd, tile);
}

// grid n_long . nft (the slots are cleared by the host before every level)
__global__ __launch_bounds__(kThreads) void forest_scan_kernel(const FitArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const Lds h = gae::cells::carve(lds, a.ft, a.bins, a.t);
    const int tile = blockIdx.x % a.nft, slot = blockIdx.x / a.nft;
    const Node nd = node_of(a, a.split_cur[slot]);
    gae::cells::load_slot<false>(a, h, a.t, nd, slot, tile);
    gae::cells::scan_tile(a, h, Variance{a, nd.at}, nd, tile);
}

// one block per tree
__global__ __launch_bounds__(kThreads) void forest_decide_kernel(const FitArgs a)
{
    __shared__ int w[kWaves];
    const int tree = blockIdx.x, tid = threadIdx.x, t = a.t;
    TreeInfo ti = a.info[tree];
    const int base = a.n_nodes[tree];
    const bool deeper = a.level + 1 < a.max_depth;
    int carry = 0, tw = 0, tc = 0, tl = 0;
    for (int i0 = 0; i0 < ti.item_n; i0 += kThreads) {
        const int i = i0 + tid;
        int split = 0, node = 0, bf = -1, bb = -1, nl = 0, n = 0;
        int64_t at = 0, cbest = 0;
        double best = -1.0, parent = 0.0;
        if (i < ti.item_n) {
            const int item = ti.item_lo + i;
            node = a.items_cur[item].node;
            at = int64_t(tree) * a.M + node;
            n = a.count[at];
            for (int tile = 0; tile < a.nft; ++tile) {     // tiles ascend in f: a strict > keeps the lower feature
                const int64_t c = int64_t(item) * a.nft + tile;
                const int2 fb = a.cand_fb[c];
                if (fb.x >= 0 && a.cand_score[c] > best) { best = a.cand_score[c]; bf = fb.x; bb = fb.y; cbest = c; }
            }
            for (int j = 0; j < t; ++j) {
                const double ds = double(a.node_sum[at * t + j]);
                parent = parent + (ds * ds / double(n)) * a.scale[j];
            }
            split = (bf >= 0 && best > parent) ? 1 : 0;
        }
        int total;
        const int k = block_scan(split, w, total);
        if (split) {
            const int L = base + 2 * (carry + k);
            nl = a.cand_nl[cbest];
            if (L + 1 >= a.M || nl <= 0 || nl >= n) {
                flag(a.status, GAE_FOREST_ERR_NODE);       // cannot happen: the capacity bounds a binary tree
            } else {
                a.feature[at] = bf; a.bin[at] = bb; a.left[at] = L;
                a.threshold[at] = a.edges[int64_t(bf) * (a.bins - 1) + bb];
                a.gain[at] = best - parent;
                const int64_t lt = int64_t(tree) * a.M + L, rt = lt + 1;
                const int start = a.seg_start[at];
                a.count[lt] = nl; a.count[rt] = n - nl;
                a.seg_start[lt] = start; a.seg_start[rt] = start + nl;
                for (int j = 0; j < t; ++j) {
                    const i64 sl = a.cand_sum[cbest * t + j];
                    a.node_sum[lt * t + j] = sl;
                    a.node_sum[rt * t + j] = a.node_sum[at * t + j] - sl;
                }
                write_value(a, lt, nl);
                write_value(a, rt, n - nl);
                for (int q = 0; q < 2; ++q) {
                    const int c = q ? n - nl : nl;
                    if (deeper && c >= 2 * a.msl) {
                        ++tw;
                        tc += chunks_of(c);
                        tl += c > kSplitRows ? 1 : 0;
                    }
                }
            }
        }
        carry += total;
    }
    int sw, sc, sl;
    block_scan(tw, w, sw);
    block_scan(tc, w, sc);
    block_scan(tl, w, sl);
    if (tid == 0) {
        ti.base = base; ti.n_new = 2 * carry; ti.tot_work = sw; ti.tot_chunks = sc; ti.tot_long = sl;
        a.info[tree] = ti;
        a.n_nodes[tree] = base + 2 * carry;
    }
}

// grid n_chunks
__global__ __launch_bounds__(kThreads) void forest_partition_kernel(const FitArgs a)
{
    const Chunk ch = a.chunks_cur[blockIdx.x];
    gae::cells::partition_chunk(a, node_of(a, ch.item), ch.chunk);
}

// one block per tree
__global__ __launch_bounds__(kThreads) void forest_emit_kernel(const FitArgs a)
{
    __shared__ int w[kWaves];
    const int tree = blockIdx.x, tid = threadIdx.x;
    int pw = 0, pc = 0, pl = 0;
    for (int q = tid; q < tree; q += kThreads) {
        const TreeInfo o = a.info[q];
        pw += o.tot_work; pc += o.tot_chunks; pl += o.tot_long;
    }
    int ow, oc, ol;
    block_scan(pw, w, ow);
    block_scan(pc, w, oc);
    block_scan(pl, w, ol);
    const TreeInfo ti = a.info[tree];
    const bool deeper = a.level + 1 < a.max_depth;
    int cw = ow, cc = oc, cl = ol;
    for (int i0 = 0; i0 < ti.n_new; i0 += kThreads) {
        const int i = i0 + tid, node = ti.base + i;
        int c = 0;
        if (i < ti.n_new) c = a.count[int64_t(tree) * a.M + node];
        const int is_w = (i < ti.n_new && deeper && c >= 2 * a.msl) ? 1 : 0;
        const int nch = is_w ? chunks_of(c) : 0;
        const int is_l = (is_w && c > kSplitRows) ? 1 : 0;
        int tw, tc, tl;
        const int kw = block_scan(is_w, w, tw), kc = block_scan(nch, w, tc), kl = block_scan(is_l, w, tl);
        if (is_w) {
            const int item = cw + kw, slot = is_l ? cl + kl : -1;
            a.items_next[item] = Item{tree, node, slot, 0};
            a.curs[item] = make_int2(0, 0);
            if (is_l) a.split_next[slot] = item;
            for (int q = 0; q < nch; ++q) a.chunks_next[int64_t(cc) + kc + q] = Chunk{item, q};
        }
        cw += tw; cc += tc; cl += tl;
    }
    if (tid == 0) {
        a.info[tree].item_lo = ow;
        a.info[tree].item_n = cw - ow;
        if (tree == a.T - 1) *a.lvl = Level{cw, cc, cl, 0};
    }
}

// ------------------------------------------------------------------------------------------------------ binning
struct BinArgs {
    const float *X;
    int64_t ldx;
    int n, d, n_rows, E, ft;
    const int32_t *rows, *n_edges;
    const float *edges;
    uint8_t *codes;
    gae_forest_status *status;
};
constexpr int kBinRows = 64;

// grid ceil(n_rows / 64) . feature tiles: the tile's edge lists in LDS, a binary search per (row, feature)
__global__ __launch_bounds__(kThreads) void forest_bin_kernel(const BinArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float *ed = reinterpret_cast<float *>(lds);            // [ftw][E]
    const int nft = (a.d + a.ft - 1) / a.ft;
    const int tid = threadIdx.x, f0 = int(blockIdx.x % nft) * a.ft, ftw = min(a.ft, a.d - f0);
    for (int c = tid; c < ftw * a.E; c += kThreads) ed[c] = a.edges[int64_t(f0) * a.E + c];
    __syncthreads();
    const int64_t r0 = int64_t(blockIdx.x / nft) * kBinRows;
    const int nr = int(min(int64_t(kBinRows), a.n_rows - r0));
    int bad = 0;
    bool bad_id = false;
    for (int idx = tid; idx < nr * ftw; idx += kThreads) {
        const int r = idx / ftw, fl = idx % ftw, f = f0 + fl;
        const int row = a.rows ? a.rows[r0 + r] : int(r0 + r);
        int code = 0;
        if (unsigned(row) >= unsigned(a.n)) {
            bad_id = true;
        } else {
            const float x = a.X[int64_t(row) * a.ldx + f];
            if (!(fabsf(x) <= FLT_MAX)) {
                ++bad;
            } else {
                int lo = 0, hi = min(a.n_edges[f], a.E);
                hi = hi < 0 ? 0 : hi;
                const float *e = ed + fl * a.E;
                while (lo < hi) {                          // lo = #{edges < x}
                    const int mid = (lo + hi) >> 1;
                    if (e[mid] < x) lo = mid + 1;
                    else hi = mid;
                }
                code = lo;
            }
        }
        a.codes[(r0 + r) * a.d + f] = uint8_t(code);
    }
    if (bad) count_nonfinite(a.status, bad);
    if (bad_id) flag(a.status, GAE_FOREST_ERR_ROW_ID);
}

// ------------------------------------------------------------------------------------------------------ predict
struct PredictArgs {
    const float *X;
    int64_t ldx;
    int m, d, t, T, M;
    const int32_t *feature, *left;
    const float *threshold;
    const double *value;
    const uint8_t *skip;
    double *out;
    gae_forest_status *status;
};

__global__ __launch_bounds__(kThreads) void forest_predict_kernel(const PredictArgs a)
{
    const int64_t row = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (row >= a.m) return;
    const float *x = a.X + row * a.ldx;
    const double nan = __builtin_nan("");
    bool finite = true;
    for (int f = 0; f < a.d; ++f) finite = finite && (fabsf(x[f]) <= FLT_MAX);
    double acc[kMaxT];
#pragma unroll
    for (int j = 0; j < kMaxT; ++j) acc[j] = 0.0;
    int used = 0;
    bool broken = false;
    if (finite) {
        for (int tree = 0; tree < a.T; ++tree) {
            if (a.skip && a.skip[int64_t(tree) * a.m + row]) continue;
            const int64_t t0 = int64_t(tree) * a.M;
            const int node = gae::cells::walk(a.feature + t0, a.left + t0, a.threshold + t0, x, a.d, a.M, kWalkSteps);
            if (node < 0) { broken = true; continue; }
#pragma unroll
            for (int j = 0; j < kMaxT; ++j)
                if (j < a.t) acc[j] += a.value[(t0 + node) * a.t + j];
            ++used;
        }
    } else {
        count_nonfinite(a.status, 1);
    }
    if (broken) flag(a.status, GAE_FOREST_ERR_NODE);
#pragma unroll
    for (int j = 0; j < kMaxT; ++j)
        if (j < a.t) a.out[row * a.t + j] = (used > 0 && !broken) ? acc[j] / double(used) : nan;
}

// ------------------------------------------------------------------------------------------------------ host
struct Plan {
    int64_t M, max_items, max_chunks, max_long, ft, nft, need;
    int32_t *pos[2], *split[2];                             // the ping-pong halves of the level lists, each pair one region
    Item *items[2];
    Chunk *chunks[2];
};

int64_t node_capacity(int64_t n_boot, int64_t max_depth)
{
    const int64_t by_depth = (int64_t(1) << (max_depth + 1)) - 1, by_rows = 2 * n_boot - 1;
    return by_depth < by_rows ? by_depth : by_rows;
}

// the checks, the sizes and THE workspace layout: on ws = NULL the regions are only counted (p.need), on the caller's buffer
// they are bound into `a` and the halves of `p`
int plan(const char *fn, int64_t n_used, int64_t d, int64_t t, int64_t T, int64_t n_boot, int64_t max_depth, int64_t bins,
         void *ws, Plan &p, FitArgs &a)
{
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..256", fn, (long long)d);
    GAE_REQUIRE(t >= 1 && t <= kMaxT, GAE_E_RANGE, "%s: t = %lld outside 1..8", fn, (long long)t);
    GAE_REQUIRE(T >= 1 && T <= kMaxTrees, GAE_E_RANGE, "%s: n_trees = %lld outside 1..1024", fn, (long long)T);
    GAE_REQUIRE(max_depth >= 1 && max_depth <= kMaxDepth, GAE_E_RANGE, "%s: max_depth = %lld outside 1..16", fn,
                (long long)max_depth);
    GAE_REQUIRE(bins >= 2 && bins <= kMaxBins, GAE_E_RANGE, "%s: max_bins = %lld outside 2..256", fn, (long long)bins);
    GAE_REQUIRE(n_used >= 1 && n_boot >= 1, GAE_E_SIZE, "%s: n_used = %lld, n_boot = %lld: at least one row", fn,
                (long long)n_used, (long long)n_boot);
    GAE_REQUIRE(n_used < (int64_t(1) << 31) && n_boot < (int64_t(1) << 31), GAE_E_SIZE,
                "%s: n_used = %lld, n_boot = %lld beyond int32 row ids", fn, (long long)n_used, (long long)n_boot);
    p.M = node_capacity(n_boot, max_depth);
    p.max_items = T * ((p.M + 1) / 2);                     // a level of a binary tree of M nodes holds (M + 1) / 2 at most
    p.max_chunks = p.max_items + T * cdiv(n_boot, kSplitRows);
    p.max_long = T * (n_boot / kSplitRows + 1);
    p.ft = gae::cells::tile_features(d, bins, t);
    p.nft = cdiv(d, p.ft);
    GAE_REQUIRE(p.max_chunks * p.nft < (int64_t(1) << 31), GAE_E_SIZE,
                "%s: %lld trees of %lld samples in %lld feature tiles are beyond a grid of 2^31 blocks", fn, (long long)T,
                (long long)n_boot, (long long)p.nft);
    gae::Carver c(ws);
    a.yq = c.take<i64>(n_used * t);
    a.node_sum = c.take<i64>(T * p.M * t);
    take_halves(c, p.pos, T * n_boot);
    a.seg_start = c.take<int32_t>(T * p.M);
    take_halves(c, p.items, p.max_items);
    take_halves(c, p.chunks, p.max_chunks);
    take_halves(c, p.split, p.max_long);
    a.curs = c.take<int2>(p.max_items);
    a.cand_score = c.take<double>(p.max_items * p.nft);
    a.cand_fb = c.take<int2>(p.max_items * p.nft);
    a.cand_nl = c.take<int32_t>(p.max_items * p.nft);
    a.cand_sum = c.take<i64>(p.max_items * p.nft * t);
    a.gcnt = c.take<unsigned>(p.max_long * d * bins);
    a.gsum = c.take<i64>(p.max_long * d * bins * t);
    a.info = c.take<TreeInfo>(T);
    a.lvl = c.take<Level>(1);
    p.need = c.bytes() + 256;
    return GAE_OK;
}

} // namespace

extern "C" int64_t gae_forest_workspace_bytes(int64_t n_used, int64_t d, int64_t t, int64_t n_trees, int64_t n_boot,
                                              int64_t max_depth, int64_t max_bins)
{
    Plan p;
    FitArgs a;
    if (const int rc = plan("gae_forest_workspace_bytes", n_used, d, t, n_trees, n_boot, max_depth, max_bins, nullptr, p, a))
        return rc;
    return p.need;
}

extern "C" int gae_forest_bin(const float *X, int64_t ldx, int64_t n, int64_t d, const int32_t *rows, int64_t n_rows,
                              const float *edges, const int32_t *n_edges, int64_t max_bins, uint8_t *codes_out,
                              gae_forest_status *status, void *stream)
{
    const char *fn = "gae_forest_bin";
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..256", fn, (long long)d);
    GAE_REQUIRE(max_bins >= 2 && max_bins <= kMaxBins, GAE_E_RANGE, "%s: max_bins = %lld outside 2..256", fn,
                (long long)max_bins);
    GAE_REQUIRE(n >= 0 && n_rows >= 0, GAE_E_SIZE, "%s: negative n = %lld or n_rows = %lld", fn, (long long)n,
                (long long)n_rows);
    GAE_REQUIRE(n < (int64_t(1) << 31) && n_rows < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld, n_rows = %lld beyond int32 row ids",
                fn, (long long)n, (long long)n_rows);
    GAE_REQUIRE(ldx >= d, GAE_E_SIZE, "%s: ldx = %lld < d = %lld", fn, (long long)ldx, (long long)d);
    GAE_REQUIRE(rows || n_rows == n, GAE_E_SIZE, "%s: rows is NULL (rows 0 .. n - 1) with n_rows = %lld, n = %lld", fn,
                (long long)n_rows, (long long)n);
    GAE_REQUIRE(edges && n_edges && status, GAE_E_NULL, "%s: edges / n_edges / status is NULL", fn);
    GAE_REQUIRE(n_rows == 0 || (X && codes_out), GAE_E_NULL, "%s: X / codes_out is NULL", fn);
    if (n_rows == 0) return GAE_OK;
    BinArgs a;
    a.X = X; a.ldx = ldx; a.n = int(n); a.d = int(d); a.n_rows = int(n_rows); a.E = int(max_bins - 1);
    a.ft = int(16384 / a.E);
    a.ft = a.ft > int(d) ? int(d) : a.ft;
    a.rows = rows; a.n_edges = n_edges; a.edges = edges; a.codes = codes_out; a.status = status;
    return gae::launch_lds<&forest_bin_kernel>("forest_bin_kernel", cdiv(n_rows, kBinRows) * cdiv(d, a.ft), kThreads,
                                               size_t(a.ft) * a.E * 4, gae::as_stream(stream), a);
}

extern "C" int gae_forest_fit(const uint8_t *codes, const int32_t *n_edges, const float *edges, int64_t n_used, int64_t d,
                              int64_t max_bins, const float *Y, int64_t ldy, int64_t n, int64_t t, const int32_t *rows,
                              const float *pivot, const int32_t *exponent, int64_t n_trees, int64_t n_boot,
                              int64_t max_depth, int64_t max_features, int64_t min_samples_leaf, int flags, uint64_t seed,
                              int32_t *feature, int32_t *threshold_bin, float *threshold, int32_t *left, int32_t *count,
                              double *value, double *gain, int32_t *n_nodes, int64_t node_capacity_, uint8_t *inbag,
                              gae_forest_status *status, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_forest_fit";
    Plan p;
    FitArgs a;
    if (const int rc = plan(fn, n_used, d, t, n_trees, n_boot, max_depth, max_bins, workspace, p, a)) return rc;
    GAE_REQUIRE(max_features >= 1 && max_features <= d, GAE_E_RANGE, "%s: max_features = %lld outside 1..d = %lld", fn,
                (long long)max_features, (long long)d);
    GAE_REQUIRE(min_samples_leaf >= 1 && min_samples_leaf < (int64_t(1) << 30), GAE_E_RANGE,
                "%s: min_samples_leaf = %lld outside 1..2^30", fn, (long long)min_samples_leaf);
    GAE_REQUIRE((flags & ~GAE_FOREST_BOOTSTRAP) == 0, GAE_E_RANGE, "%s: unknown flags 0x%x", fn, flags);
    GAE_REQUIRE((flags & GAE_FOREST_BOOTSTRAP) || n_boot == n_used, GAE_E_SIZE,
                "%s: without the bootstrap n_boot = %lld must equal n_used = %lld", fn, (long long)n_boot, (long long)n_used);
    GAE_REQUIRE(n >= 0 && n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld outside 0..2^31", fn, (long long)n);
    GAE_REQUIRE(ldy >= t, GAE_E_SIZE, "%s: ldy = %lld < t = %lld", fn, (long long)ldy, (long long)t);
    GAE_REQUIRE(rows || n_used == n, GAE_E_SIZE, "%s: rows is NULL (rows 0 .. n - 1) with n_used = %lld, n = %lld", fn,
                (long long)n_used, (long long)n);
    GAE_REQUIRE(node_capacity_ == p.M, GAE_E_SIZE, "%s: node_capacity = %lld, min(2^(max_depth + 1) - 1, 2 n_boot - 1) = %lld", fn,
                (long long)node_capacity_, (long long)p.M);
    GAE_REQUIRE(codes && n_edges && edges && Y && pivot && exponent, GAE_E_NULL,
                "%s: codes / n_edges / edges / Y / pivot / exponent is NULL", fn);
    GAE_REQUIRE(feature && threshold_bin && threshold && left && count && value && gain && n_nodes && status, GAE_E_NULL,
                "%s: an output or status is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(workspace_bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)p.need);
    for (int j = 0; j < t; ++j)
        GAE_REQUIRE(exponent[j] >= -200 && exponent[j] <= 200 && fabsf(pivot[j]) <= FLT_MAX, GAE_E_RANGE,
                    "%s: exponent[%d] = %d outside -200..200 or a non-finite pivot", fn, j, exponent[j]);

    a.codes = codes; a.n_edges = n_edges; a.edges = edges; a.Y = Y; a.rows = rows; a.ldy = ldy;
    a.n = int(n); a.n_used = int(n_used); a.d = int(d); a.t = int(t); a.bins = int(max_bins); a.T = int(n_trees);
    a.n_boot = int(n_boot); a.max_depth = int(max_depth); a.m_feat = int(max_features); a.msl = int(min_samples_leaf);
    a.bootstrap = (flags & GAE_FOREST_BOOTSTRAP) ? 1 : 0; a.M = int(p.M); a.ft = int(p.ft); a.nft = int(p.nft); a.level = 0;
    a.key = seed ^ GAE_FOREST_KEY_XOR;
    for (int j = 0; j < kMaxT; ++j) {
        const int e = j < t ? exponent[j] : 0;
        a.pivot[j] = j < t ? pivot[j] : 0.f;
        a.up[j] = ldexp(1.0, e); a.inv[j] = ldexp(1.0, -e); a.scale[j] = ldexp(1.0, -2 * e);
    }
    a.feature = feature; a.bin = threshold_bin; a.left = left; a.count = count; a.n_nodes = n_nodes;
    a.threshold = threshold; a.value = value; a.gain = gain; a.inbag = inbag; a.status = status;
    auto side = [&](int cur) {
        a.pos_in = p.pos[cur]; a.pos_out = p.pos[cur ^ 1];
        a.items_cur = p.items[cur]; a.items_next = p.items[cur ^ 1];
        a.chunks_cur = p.chunks[cur]; a.chunks_next = p.chunks[cur ^ 1];
        a.split_cur = p.split[cur]; a.split_next = p.split[cur ^ 1];
    };
    side(0);
    hipStream_t st = gae::as_stream(stream);

    GAE_HIP(hipMemsetAsync(a.node_sum, 0, size_t(n_trees) * p.M * t * 8, st));
    if (inbag) GAE_HIP(hipMemsetAsync(inbag, 0, size_t(n_trees) * n_used, st));
    {
        const int64_t total = n_trees * p.M, blocks = cdiv(total, kThreads);
        hipLaunchKernelGGL(forest_fill_kernel, dim3(unsigned(blocks > 4096 ? 4096 : blocks)), dim3(kThreads), 0, st, a);
        GAE_CHECK_LAUNCH("forest_fill_kernel");
    }
    hipLaunchKernelGGL(forest_quant_kernel, dim3(unsigned(cdiv(n_used * t, kThreads))), dim3(kThreads), 0, st, a);
    GAE_CHECK_LAUNCH("forest_quant_kernel");
    hipLaunchKernelGGL(forest_boot_kernel, dim3(unsigned(cdiv(n_boot, kThreads)), unsigned(n_trees)), dim3(kThreads), 0, st, a);
    GAE_CHECK_LAUNCH("forest_boot_kernel");
    const int offered = n_boot >= 2 * min_samples_leaf ? 1 : 0;          // max_depth >= 1
    hipLaunchKernelGGL(forest_root_kernel, dim3(unsigned(cdiv(n_trees, kThreads))), dim3(kThreads), 0, st, a, offered);
    GAE_CHECK_LAUNCH("forest_root_kernel");

    Level lv = {0, 0, 0, 0};
    if (offered) {
        lv.n_items = n_trees;
        lv.n_chunks = n_trees * cdiv(n_boot, kSplitRows);
        lv.n_long = n_boot > kSplitRows ? n_trees : 0;
    }
    const size_t lds = gae::cells::lds_bytes(int(p.ft), int(max_bins), int(t));
    int cur = 0;
    for (int level = 0; level < max_depth && lv.n_items > 0; ++level) {
        GAE_REQUIRE(lv.n_items <= p.max_items && lv.n_chunks <= p.max_chunks && lv.n_long <= p.max_long && lv.n_chunks >= lv.n_items,
                    GAE_E_SIZE, "%s: level %d reports %lld nodes, %lld chunks, %lld long nodes: beyond the work lists", fn, level,
                    (long long)lv.n_items, (long long)lv.n_chunks, (long long)lv.n_long);
        a.level = level;
        side(cur);
        if (lv.n_long > 0) {
            GAE_HIP(hipMemsetAsync(a.gcnt, 0, size_t(lv.n_long) * d * max_bins * 4, st));
            GAE_HIP(hipMemsetAsync(a.gsum, 0, size_t(lv.n_long) * d * max_bins * t * 8, st));
        }
        if (const int rc = gae::launch_lds<&forest_hist_kernel>("forest_hist_kernel", lv.n_chunks * p.nft, kThreads, lds, st, a))
            return rc;
        if (lv.n_long > 0)
            if (const int rc = gae::launch_lds<&forest_scan_kernel>("forest_scan_kernel", lv.n_long * p.nft, kThreads, lds, st, a))
                return rc;
        hipLaunchKernelGGL(forest_decide_kernel, dim3(unsigned(n_trees)), dim3(kThreads), 0, st, a);
        GAE_CHECK_LAUNCH("forest_decide_kernel");
        if (level + 1 >= max_depth) break;                                 // the children are leaves: no lists, no partition
        hipLaunchKernelGGL(forest_partition_kernel, dim3(unsigned(lv.n_chunks)), dim3(kThreads), 0, st, a);
        GAE_CHECK_LAUNCH("forest_partition_kernel");
        hipLaunchKernelGGL(forest_emit_kernel, dim3(unsigned(n_trees)), dim3(kThreads), 0, st, a);
        GAE_CHECK_LAUNCH("forest_emit_kernel");
        GAE_HIP(hipMemcpyAsync(&lv, a.lvl, sizeof(Level), hipMemcpyDeviceToHost, st));      // the level's one read
        GAE_HIP(hipStreamSynchronize(st));
        cur ^= 1;
    }
    return GAE_OK;
}

extern "C" int gae_forest_predict(const float *X, int64_t ldx, int64_t m, int64_t d, int64_t t, int64_t n_trees,
                                  int64_t node_capacity_, const int32_t *feature, const float *threshold,
                                  const int32_t *left, const double *value, const uint8_t *skip, double *out,
                                  gae_forest_status *status, void *stream)
{
    const char *fn = "gae_forest_predict";
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..256", fn, (long long)d);
    GAE_REQUIRE(t >= 1 && t <= kMaxT, GAE_E_RANGE, "%s: t = %lld outside 1..8", fn, (long long)t);
    GAE_REQUIRE(n_trees >= 1 && n_trees <= kMaxTrees, GAE_E_RANGE, "%s: n_trees = %lld outside 1..1024", fn, (long long)n_trees);
    GAE_REQUIRE(m >= 0 && m < (int64_t(1) << 31), GAE_E_SIZE, "%s: m = %lld outside 0..2^31", fn, (long long)m);
    GAE_REQUIRE(node_capacity_ >= 1 && node_capacity_ < (int64_t(1) << 18), GAE_E_SIZE, "%s: node_capacity = %lld outside 1..2^18",
                fn, (long long)node_capacity_);
    GAE_REQUIRE(ldx >= d, GAE_E_SIZE, "%s: ldx = %lld < d = %lld", fn, (long long)ldx, (long long)d);
    GAE_REQUIRE(feature && threshold && left && value && status, GAE_E_NULL, "%s: a node table or status is NULL", fn);
    GAE_REQUIRE(m == 0 || (X && out), GAE_E_NULL, "%s: X / out is NULL", fn);
    if (m == 0) return GAE_OK;
    const PredictArgs a{X, ldx, int(m), int(d), int(t), int(n_trees), int(node_capacity_), feature, left, threshold, value, skip,
                        out, status};
    hipLaunchKernelGGL(forest_predict_kernel, dim3(unsigned(cdiv(m, kThreads))), dim3(kThreads), 0, gae::as_stream(stream), a);
    GAE_CHECK_LAUNCH("forest_predict_kernel");
    return GAE_OK;
}
