// What the histogram-tree families share (K26 forest.hip, K30 boost.hip): the level pass over one node's samples and one
// feature tile's LDS cells, and its small helpers.  Blocks of 256 threads.
//
// A level pass, top to bottom of this file: fill_tile (a chunk of the node's samples into the tile's count and int64-sum
// cells by integer atomics; a node longer than one chunk merges them into its global slot), load_slot (the merged cells
// back into LDS), scan_tile (prefix sums over the bins, every candidate's score, the tile's best candidate record) and
// partition_chunk (the samples of a node that split, into the other pos buffer); walk is the tree walk of the two predict
// kernels.  The families keep the __global__ kernels: each finds its block's chunk and node in its own lists, describes
// them as a Node, and says with two small policies what is its own --
//   words   int words() const                 int64 sums per cell (a compile-time constant unrolls the loops over them)
//           i64 word(int s, int j) const      word j of listed row s
//   score   int words() const
//           double score(const Lds &h, int idx, int n_left, int n_right) const
//                                             the fp64 score of the candidate at cell idx of the prefix-summed tile
//                                             (every score is >= 0), or a negative number: not a candidate
// -- the rest (set-up, the split decision, the next level's lists, the leaf values) is theirs alone.
#pragma once
#include "common.h"

namespace gae {
namespace cells {

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kHistBytes = 64 * 1024;      // LDS cells of one feature tile
constexpr int kSplitRows = GAE_FOREST_SPLIT_ROWS;

typedef unsigned long long u64;
typedef long long i64;

__host__ __device__ inline int chunks_of(int rows) { return (rows + kSplitRows - 1) / kSplitRows; }

struct Chunk { int item, chunk; };         // rows [chunk . kSplitRows, + kSplitRows) of work item `item`'s node

__device__ __forceinline__ void flag(gae_forest_status *st, int64_t bits)
{
    atomicOr(reinterpret_cast<u64 *>(&st->errors), static_cast<u64>(bits));
}
__device__ __forceinline__ void add_i64(i64 *p, i64 v) { atomicAdd(reinterpret_cast<u64 *>(p), static_cast<u64>(v)); }

// the two ping-pong halves of a level list, one workspace region
template <class T>
void take_halves(Carver &c, T *(&two)[2], int64_t half)
{
    two[0] = c.take<T>(2 * half);
    two[1] = two[0] ? two[0] + half : nullptr;
}

// exclusive scan of v over the block's 256 threads (all must call); total = the block's sum.  w: 4 ints of LDS
__device__ __forceinline__ int block_scan(int v, int *w, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    if (lane == 63) w[wave] = x;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < kWaves; ++q) {
        const int s = w[q];
        if (q < wave) base += s;
        total += s;
    }
    __syncthreads();
    return base + x - v;
}

// sel[f] = 1 for the candidate features of node `node` under the stream `draw`: all d of them when m >= d, else the m with
// the smallest (r_f, f), r_f = word 0 of philox4x32_10(ctr = (node << 8) | f, draw, key).  All 256 threads call (d <= 256 =
// the block); rkey: 256 words of LDS, sel: 256 bytes.  Ends in a barrier
__device__ __forceinline__ void select_subset(unsigned char *sel, unsigned *rkey, int d, int m, int node, uint64_t draw,
                                              uint64_t key)
{
    const int f = threadIdx.x;
    if (m >= d) {
        sel[f] = 1;
        __syncthreads();
        return;
    }
    if (f < d) {
        uint32_t c[4];
        philox4x32_10((uint64_t(node) << 8) | uint64_t(f), draw, key, c);
        rkey[f] = c[0];
    }
    __syncthreads();
    if (f < d) {
        const unsigned mine = rkey[f];
        int rank = 0;
        for (int g = 0; g < d; ++g) {
            const unsigned other = rkey[g];
            rank += (other < mine || (other == mine && g < f)) ? 1 : 0;
        }
        sel[f] = rank < m ? 1 : 0;
    } else {
        sel[f] = 0;
    }
    __syncthreads();
}

// candidate (s, f, b) beats (s2, f2, b2): the larger score, then the lower feature, then the lower bin
__device__ __forceinline__ bool better(double s, int f, int b, double s2, int f2, int b2)
{
    return s > s2 || (s == s2 && (f < f2 || (f == f2 && b < b2)));
}

// One feature tile in LDS: u32 counts [cells], then `words` int64 sums per cell, then the block's reduction scratch
// (score, feature, bin per thread), the Philox words and the subset marks
struct Lds {
    unsigned *cnt;                         // [ft][bins]
    long long *sum;                        // [ft][bins][words]
    double *rs;                            // [256] reduction: score, feature, bin
    int *rf, *rb;
    unsigned *rkey;                        // [256] Philox words of the feature subset
    unsigned char *sel;                    // [256]
};

__host__ __device__ inline size_t lds_bytes(int ft, int bins, int words)
{
    const size_t cells = size_t(ft) * bins;
    return (cells * 4 + 7) / 8 * 8 + cells * words * 8 + kThreads * (8 + 4 + 4 + 4 + 1);
}

// features per tile: as many as kHistBytes of cells hold, 1 at least, d at most
__host__ __device__ inline int64_t tile_features(int64_t d, int64_t bins, int64_t words)
{
    const int64_t ft = kHistBytes / (bins * (4 + 8 * words));
    return ft < 1 ? 1 : (ft > d ? d : ft);
}

__device__ __forceinline__ Lds carve(unsigned char *lds, int ft, int bins, int words)
{
    Lds h;
    const size_t cells = size_t(ft) * bins;
    h.cnt = reinterpret_cast<unsigned *>(lds);
    h.sum = reinterpret_cast<long long *>(lds + (cells * 4 + 7) / 8 * 8);
    h.rs = reinterpret_cast<double *>(h.sum + cells * words);
    h.rf = reinterpret_cast<int *>(h.rs + kThreads);
    h.rb = h.rf + kThreads;
    h.rkey = reinterpret_cast<unsigned *>(h.rb + kThreads);
    h.sel = reinterpret_cast<unsigned char *>(h.rkey + kThreads);
    return h;
}

// ------------------------------------------------------------------------------------------------------ a level
// What a level pass reads and writes in either family: the base of the family's kernel arguments.  Every array is the
// family's whole region; a Node says where a block's part of it starts
struct Frame {
    const uint8_t *codes;                  // [n_used][d]
    const int32_t *n_edges;                // [d]
    int n_used, d, bins, ft, nft, m_feat, msl;
    uint64_t key;
    gae_forest_status *status;
    int32_t *feature, *bin, *left, *count, *seg_start;     // node tables, M rows per tree or model
    int32_t *pos_in, *pos_out;             // the level's sample lists and the next level's
    int2 *curs;                            // per work item: the left and right cursors of the partition
    unsigned *gcnt;                        // per long-node slot [d][bins]
    i64 *gsum;                             // [d][bins][words]
    double *cand_score;                    // per (work item, feature tile): the tile's best candidate
    int2 *cand_fb;
    int32_t *cand_nl;
    i64 *cand_sum;                         // [words] the left sums
};

struct Node {
    int64_t at;                            // its row of the node tables
    int64_t rows;                          // where its tree's or model's list starts in pos_in / pos_out
    int64_t item;                          // its work item: curs[item], candidate records item . nft + tile
    int64_t slot;                          // a node longer than one chunk: its cells in gcnt / gsum; else < 0
    int node;                              // its number in its tree: the counter of its feature subset ...
    uint64_t draw;                         // ... and the subset's Philox stream
};

// The cells of features [tile . ft, ...) over chunk ch of the node, in LDS.  True: the node is longer than one chunk, the
// cells went to its slot and load_slot + scan_tile follow in another launch; false: they are the node's, scan_tile follows
template <class Words>
__device__ __forceinline__ bool fill_tile(const Frame &a, const Lds &h, const Words &p, const Node &nd, Chunk ch, int tile)
{
    const int tid = threadIdx.x, bins = a.bins, W = p.words();
    const int f0 = tile * a.ft, ftw = min(a.ft, a.d - f0), cells = ftw * bins;
    const int start = a.seg_start[nd.at], n = a.count[nd.at];
    const int r0 = ch.chunk * kSplitRows, nr = min(n - r0, kSplitRows);
    for (int c = tid; c < cells; c += kThreads) h.cnt[c] = 0u;
    for (int c = tid; c < cells * W; c += kThreads) h.sum[c] = 0;
    select_subset(h.sel, h.rkey, a.d, a.m_feat, nd.node, nd.draw, a.key);      // (its barrier also covers the zeroing)
    const int32_t *pos = a.pos_in + nd.rows + start + r0;
    bool bad = false;
    for (int idx = tid; idx < nr * ftw; idx += kThreads) {      // <= 8192 . 256
        const int r = idx / ftw, fl = idx % ftw;
        if (!h.sel[f0 + fl]) continue;
        const int s = pos[r];
        if (unsigned(s) >= unsigned(a.n_used)) { bad = true; continue; }       // (cannot happen: the lists hold listed rows)
        const int code = a.codes[int64_t(s) * a.d + f0 + fl];
        if (code >= bins) { bad = true; continue; }
        const int cell = fl * bins + code;
        atomicAdd(&h.cnt[cell], 1u);
        for (int j = 0; j < W; ++j) add_i64(&h.sum[cell * W + j], p.word(s, j));
    }
    if (bad) flag(a.status, GAE_FOREST_ERR_CODE);
    __syncthreads();
    if (nd.slot < 0) return false;
    const int64_t g0 = (nd.slot * a.d + f0) * bins;
    for (int c = tid; c < cells; c += kThreads) {
        const unsigned v = h.cnt[c];
        if (!v) continue;
        atomicAdd(&a.gcnt[g0 + c], v);
        for (int j = 0; j < W; ++j) add_i64(&a.gsum[(g0 + c) * W + j], h.sum[c * W + j]);
    }
    return true;
}

// The merged cells of slot `slot`, tile `tile`, into LDS (kLeaveZeroed: and the slot ready for its next user), and the
// node's feature subset.  Ends in a barrier
template <bool kLeaveZeroed>
__device__ __forceinline__ void load_slot(const Frame &a, const Lds &h, int W, const Node &nd, int64_t slot, int tile)
{
    const int tid = threadIdx.x;
    const int f0 = tile * a.ft, ftw = min(a.ft, a.d - f0), cells = ftw * a.bins;
    const int64_t g0 = (slot * a.d + f0) * a.bins;
    for (int c = tid; c < cells; c += kThreads) {
        h.cnt[c] = a.gcnt[g0 + c];
        if (kLeaveZeroed) a.gcnt[g0 + c] = 0u;
    }
    for (int c = tid; c < cells * W; c += kThreads) {
        h.sum[c] = a.gsum[g0 * W + c];
        if (kLeaveZeroed) a.gsum[g0 * W + c] = 0;
    }
    select_subset(h.sel, h.rkey, a.d, a.m_feat, nd.node, nd.draw, a.key);
}

// The node's cells of the tile are in LDS: prefix sums over the bins, every candidate's score, the tile's best candidate
// (score; feature and bin, or (-1, -1); the left count and the left sums) to the node's record of this tile
template <class Score>
__device__ __forceinline__ void scan_tile(const Frame &a, const Lds &h, const Score &p, const Node &nd, int tile)
{
    const int tid = threadIdx.x, bins = a.bins, W = p.words();
    const int f0 = tile * a.ft, ftw = min(a.ft, a.d - f0);
    for (int q = tid; q < ftw * (W + 1); q += kThreads) {
        const int fl = q / (W + 1), w = q % (W + 1);
        if (w == 0) {
            unsigned run = 0;
            for (int b = 0; b < bins; ++b) { run += h.cnt[fl * bins + b]; h.cnt[fl * bins + b] = run; }
        } else {
            i64 run = 0;
            for (int b = 0; b < bins; ++b) { run += h.sum[(fl * bins + b) * W + (w - 1)]; h.sum[(fl * bins + b) * W + (w - 1)] = run; }
        }
    }
    __syncthreads();
    const int n = a.count[nd.at];
    double bs = -1.0;                      // every score is >= 0
    int bf = 0x7fffffff, bb = 0x7fffffff;
    for (int idx = tid; idx < ftw * bins; idx += kThreads) {
        const int fl = idx / bins, b = idx % bins, f = f0 + fl;
        if (b >= min(a.n_edges[f], bins - 1) || !h.sel[f]) continue;
        const int nl = int(h.cnt[idx]), nr = n - nl;
        if (nl < a.msl || nr < a.msl) continue;
        const double score = p.score(h, idx, nl, nr);
        if (score < 0.0) continue;
        if (better(score, f, b, bs, bf, bb)) { bs = score; bf = f; bb = b; }
    }
    h.rs[tid] = bs; h.rf[tid] = bf; h.rb[tid] = bb;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off && better(h.rs[tid + off], h.rf[tid + off], h.rb[tid + off], h.rs[tid], h.rf[tid], h.rb[tid])) {
            h.rs[tid] = h.rs[tid + off]; h.rf[tid] = h.rf[tid + off]; h.rb[tid] = h.rb[tid + off];
        }
        __syncthreads();
    }
    const int64_t c = nd.item * a.nft + tile;
    const bool found = h.rs[0] >= 0.0;
    const int cell = found ? (h.rf[0] - f0) * bins + h.rb[0] : 0;
    if (tid == 0) {
        a.cand_score[c] = h.rs[0];
        a.cand_fb[c] = found ? make_int2(h.rf[0], h.rb[0]) : make_int2(-1, -1);
        a.cand_nl[c] = found ? int(h.cnt[cell]) : 0;
    }
    if (tid < W) a.cand_sum[c * W + tid] = found ? h.sum[cell * W + tid] : 0;
}

// Rows [chunk . kSplitRows, ...) of a node that split, from its segment of pos_in into its children's segments of
// pos_out; the chunks of a node reserve their ranges with the work item's two cursors (the order inside a segment is not
// part of any result).  A leaf's segment is never read again
__device__ __forceinline__ void partition_chunk(const Frame &a, const Node &nd, int chunk)
{
    __shared__ int w[kWaves];
    __shared__ int bases[2];
    const int tid = threadIdx.x;
    const int f = a.feature[nd.at];
    if (f < 0) return;
    const int b = a.bin[nd.at], n = a.count[nd.at], start = a.seg_start[nd.at];
    const int nl = a.count[nd.at - nd.node + a.left[nd.at]], nrt = n - nl;
    const int r0 = chunk * kSplitRows, r1 = min(n, r0 + kSplitRows);
    const int32_t *src = a.pos_in + nd.rows + start;
    int32_t *dst = a.pos_out + nd.rows + start;
    bool bad = false;
    for (int i0 = r0; i0 < r1; i0 += kThreads) {
        const int r = i0 + tid;
        const bool on = r < r1;
        int s = on ? src[r] : 0;
        if (unsigned(s) >= unsigned(a.n_used)) { bad = true; s = 0; }
        const int goes_left = (on && a.codes[int64_t(s) * a.d + f] <= b) ? 1 : 0;
        int totl;
        const int kl = block_scan(goes_left, w, totl);
        if (tid == 0) {
            const int live = min(kThreads, r1 - i0);
            bases[0] = atomicAdd(&a.curs[nd.item].x, totl);
            bases[1] = atomicAdd(&a.curs[nd.item].y, live - totl);
        }
        __syncthreads();
        if (on) {
            const int o = goes_left ? bases[0] + kl : bases[1] + (tid - kl);
            if (goes_left ? o < nl : o < nrt) dst[goes_left ? o : nl + o] = s;
            else bad = true;
        }
        __syncthreads();
    }
    if (bad) flag(a.status, GAE_FOREST_ERR_NODE);
}

// ------------------------------------------------------------------------------------------------------ predict
// The leaf that row x reaches in one tree's tables (M rows; x[f] <= threshold goes left), or -1 for a broken table: a
// feature >= d, a child outside 1 .. M - 2, more than max_steps steps
__device__ __forceinline__ int walk(const int32_t *feature, const int32_t *left, const float *threshold, const float *x, int d,
                                    int M, int max_steps)
{
    int node = 0, steps = 0;
    while (true) {
        const int f = feature[node];
        if (f < 0) return node;
        const int L = left[node];
        if (f >= d || L < 1 || L + 1 >= M || ++steps > max_steps) return -1;
        node = L + (x[f] <= threshold[node] ? 0 : 1);
    }
}

} // namespace cells
} // namespace gae
