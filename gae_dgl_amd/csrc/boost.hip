// K30: second-order histogram gradient boosting on frozen features (ops.boost, GAE.boost_graphs, embed --boost).
//
// The contract -- the fixed-point frame of g and h, the restated sigma, the round prologue, the split score and its order
// of operations, the tie rules, node numbering, leaf weights, the held-out loss and its order, prediction, the status
// block -- is the K30 comment of include/gae_hip_experimental.h.  Every accumulated quantity is an integer (bin codes,
// int64 fixed-point gradients and Hessians, integer counts and sums), so integer atomics in LDS and in global memory are
// exact and free of order.  This file is built with -ffp-contract=off (_build.py): every fp64 step is a plain IEEE
// operation that numpy restates one to one (tests/boost_ref.py).
//
// MODELS  model m = cfg (folds + 1) + k: k < folds is the model that holds fold k out, k == folds the all-rows model.
// LAYOUTS
//   codes     uint8 [n_used][d], row-major by listed row (gae_forest_bin)
//   score     fp64 [models][n_used], the running score F (an output: its final value is the fit's raw score)
//   gq, hq    int64 [models][n_used], this round's fixed-point g and h
//   pos       int32 [models][n_used], two buffers: a model's training rows, kept partitioned by node after every level
//   tables    [models][M] scratch node tables of the round's trees; the all-rows models' are copied out after the round
//   lists     per model a FIXED region of the level's work items (<= 2^(depth - 1)), chunks (items + ceil(n_used /
//             GAE_FOREST_SPLIT_ROWS)) and long-node slots (n_used / GAE_FOREST_SPLIT_ROWS), two buffers, with a 16-byte
//             level record per model that stays on the device
// LAUNCHES of one round, all models at once, every grid sized by its bound (surplus blocks return at once):
//   prologue  (256-row chunk, model): F += the last tree's leaf, g and h, the sample list and the root sums by integer
//             atomics, the chunk's held-out loss in a fixed order
//   root      one block per model: folds the loss chunks, resets the model's table, node 0, the level-0 lists
//   then per level: hist (chunk, feature tile, model), scan (long node, feature tile, model; only when n_used exceeds a
//   chunk), decide (model: the split test, the children, the next level's lists), partition (chunk, model; not after the
//   last level); and keep (configuration): the all-rows model's table to the output.  The bodies of hist, scan and
//   partition and the tree walk of predict are the level pass of forest_cells.h, K26's too; what is boost's own there is
//   its lists (node_of) and the GradHess and Gain policies.
// After the last round one more prologue + root give the final score and the last point of the loss curve.  The host
// reads the 32-byte status once per check_every rounds and once at the end; nothing else synchronises.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "common.h"
#include "forest_cells.h"
#include "sigma64.h"

namespace {

using gae::cdiv;
using gae::cells::add_i64;
using gae::cells::block_scan;
using gae::cells::Chunk;
using gae::cells::chunks_of;
using gae::cells::flag;
using gae::cells::i64;
using gae::cells::take_halves;
using gae::cells::u64;

constexpr int kMaxD = 256, kMaxBins = 256, kMaxDepth = 8, kMaxRounds = 4096, kMaxModels = 256;
constexpr int kSplitRows = gae::cells::kSplitRows;
constexpr int kThreads = gae::cells::kThreads, kWaves = gae::cells::kWaves;
constexpr int kLossRows = 256;             // rows per held-out loss partial = the prologue's block

struct Item { int node, slot; };           // slot >= 0: a node longer than one chunk, its global cells
struct Level { int n_items, n_chunks, n_long, pad; };

struct Args : gae::cells::Frame {                          // (the level pass's own arrays are the Frame's)
    const float *edges;
    const float *y;
    const int32_t *fold;
    int folds, n_cfg, Mo, depth, M, objective, R, maxI, maxC, maxL, n_parts;
    int round, level, gx, gl;              // gx, gl: blocks per model of this level's hist and scan launches
    double mcw, min_gain, base, g_up, g_step, h_up, h_step;
    const double *lr, *lam;                // [n_cfg] (workspace)
    // outputs
    int32_t *o_feature, *o_bin, *o_left, *o_count, *o_n_nodes;
    float *o_threshold;
    double *o_value, *o_gain, *loss, *score;
    i64 *correct;
    int32_t *bad;
    // workspace
    int32_t *n_nodes;
    float *threshold;
    double *value, *gain;
    i64 *nG, *nH, *gq, *hq, *root;
    int32_t *split_cur, *split_next;
    Item *items_cur, *items_next;
    Chunk *chunks_cur, *chunks_next;
    int2 *curs_next;
    Level *lvl_cur, *lvl_next;
    double *part;
};

// a model left the fixed-point frame or went non-finite: marked once, counted once in status.reserved[0]
__device__ __forceinline__ void mark_bad(const Args &a, int m)
{
    if (atomicExch(&a.bad[m], 1) == 0) add_i64(reinterpret_cast<i64 *>(&a.status->reserved[0]), 1);
}

// ------------------------------------------------------------------------------------------------------ sigma
// the stated fp64 sequence of sigma64.h (shared with K38): exp(-min(|F|, 40)), then q = e / (1 + e) or 1 - q
using gae::sigma64::clamp_abs;
using gae::sigma64::exp_neg;
using gae::sigma64::sigma_of;

// ------------------------------------------------------------------------------------------------------ a round
__device__ __forceinline__ double leaf_weight(const Args &a, i64 G, i64 H, double lr, double lam)
{
    const double g = double(G) * a.g_step, den = double(H) * a.h_step + lam;
    return den > 0.0 ? -(lr * (g / den)) : 0.0;
}

__device__ __forceinline__ i64 quantise(const Args &a, int m, double v, bool on)
{
    if (!on) return 0;
    if (!(fabs(v) <= 2147483648.0)) {      // beyond the frame (or NaN): the model is marked, nothing wraps
        mark_bad(a, m);
        return 0;
    }
    return llrint(v);
}

// grid (n_parts, models)
__global__ __launch_bounds__(kThreads) void boost_prologue_kernel(const Args a)
{
    __shared__ int w[kWaves];
    __shared__ double sl[kWaves];
    __shared__ int base_s;
    const int m = blockIdx.y, k = m % (a.folds + 1), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * kThreads + tid;
    const bool on = i < a.n_used;
    const int64_t at = int64_t(m) * a.n_used + i;
    double F = a.base;
    if (on && a.round > 0) {
        const uint8_t *c = a.codes + int64_t(i) * a.d;
        const int64_t tb = int64_t(m) * a.M;
        int node = 0;
        for (int step = 0; step < kMaxDepth; ++step) {
            const int f = a.feature[tb + node];
            if (f < 0) break;
            node = a.left[tb + node] + (int(c[f]) <= a.bin[tb + node] ? 0 : 1);
        }
        F = a.score[at] + a.value[tb + node];
    }
    if (on) a.score[at] = F;
    const float yf = on ? a.y[i] : 0.f;
    const double yd = double(yf);
    const int fo = (on && a.fold) ? a.fold[i] : -1;
    if (on && a.round == 0 && m == 0) {
        if (a.objective == GAE_BOOST_LOGISTIC ? !(yf == 0.f || yf == 1.f) : !(fabsf(yf) <= FLT_MAX))
            flag(a.status, GAE_BOOST_ERR_TARGET);
        if (a.folds > 0 && unsigned(fo) >= unsigned(a.folds)) flag(a.status, GAE_BOOST_ERR_FOLD);
    }
    if (on && !(fabs(F) <= DBL_MAX)) mark_bad(a, m);
    const bool held = on && k < a.folds && fo == k;
    const bool train = on && !held && a.round < a.R;
    double g, h = 1.0, loss;
    int right = 0;
    if (a.objective == GAE_BOOST_LOGISTIC) {
        const double e = exp_neg(clamp_abs(F));
        const double p = sigma_of(F, e);
        g = p - yd;
        h = p * (1.0 - p);
        const bool up = F >= 0.0, one = yf > 0.5f;
        loss = log1p(e) + (up == one ? 0.0 : fabs(F));
        right = up == one ? 1 : 0;
    } else {
        g = F - yd;
        loss = g * g;
    }
    const i64 gq = quantise(a, m, g * a.g_up, train);
    const i64 hq = a.objective == GAE_BOOST_LOGISTIC ? quantise(a, m, h * a.h_up, train) : (train ? 1 : 0);
    int tot;
    const int kp = block_scan(train ? 1 : 0, w, tot);
    if (tid == 0) base_s = tot ? int(atomicAdd(reinterpret_cast<u64 *>(&a.root[m * 4]), static_cast<u64>(tot))) : 0;
    __syncthreads();
    if (train) {
        a.pos_in[int64_t(m) * a.n_used + base_s + kp] = i;
        a.gq[at] = gq;
        a.hq[at] = hq;
    }
    i64 sg = gq, sh = hq;
    double lsum = held ? loss : 0.0;
    int ok = held ? right : 0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sg += __shfl_down(sg, off, 64);
        sh += __shfl_down(sh, off, 64);
        lsum += __shfl_down(lsum, off, 64);
        ok += __shfl_down(ok, off, 64);
    }
    if (lane == 0) {
        if (sg) add_i64(&a.root[m * 4 + 1], sg);
        if (sh) add_i64(&a.root[m * 4 + 2], sh);
        if (ok) add_i64(&a.correct[int64_t(m) * (a.R + 1) + a.round], ok);
        sl[wave] = lsum;
    }
    __syncthreads();
    if (tid == 0) a.part[int64_t(m) * a.n_parts + blockIdx.x] = ((sl[0] + sl[1]) + sl[2]) + sl[3];
}

// the order of common.h's sum_partials on doubles: lists of <= 32 one lane, longer lists 64 lanes and the shuffle tree
__device__ __forceinline__ double fold_partials(const double *p, int n, int lane)
{
    const int L = n > 32 ? 64 : 1;
    double g = 0.0;
    if (lane < L)
        for (int q = lane; q < n; q += L) g += p[q];
    if (L == 64) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) g += __shfl_down(g, off, 64);
    }
    return g;
}

// one block per model
__global__ __launch_bounds__(kThreads) void boost_root_kernel(const Args a)
{
    const int m = blockIdx.x, tid = threadIdx.x, cfg = m / (a.folds + 1);
    if (tid < 64) {
        const double v = fold_partials(a.part + int64_t(m) * a.n_parts, a.n_parts, tid);
        if (tid == 0) a.loss[int64_t(m) * (a.R + 1) + a.round] = v;
    }
    if (a.round >= a.R) return;
    const i64 n = a.root[m * 4], G = a.root[m * 4 + 1], H = a.root[m * 4 + 2];
    const int64_t tb = int64_t(m) * a.M;
    for (int j = tid; j < a.M; j += kThreads) {
        a.feature[tb + j] = -1; a.bin[tb + j] = -1; a.left[tb + j] = -1; a.count[tb + j] = 0; a.seg_start[tb + j] = 0;
        a.threshold[tb + j] = 0.f; a.value[tb + j] = 0.0; a.gain[tb + j] = 0.0; a.nG[tb + j] = 0; a.nH[tb + j] = 0;
    }
    const bool offered = n >= 2 * i64(a.msl);
    const int nch = chunks_of(int(n));
    const bool is_long = n > kSplitRows;
    if (offered)
        for (int c = tid; c < nch; c += kThreads) a.chunks_cur[int64_t(m) * a.maxC + c] = Chunk{0, c};
    __syncthreads();
    if (tid == 0) {
        a.count[tb] = int(n); a.nG[tb] = G; a.nH[tb] = H;
        a.value[tb] = leaf_weight(a, G, H, a.lr[cfg], a.lam[cfg]);
        a.n_nodes[m] = 1;
        a.items_cur[int64_t(m) * a.maxI] = Item{0, is_long ? 0 : -1};
        a.curs[int64_t(m) * a.maxI] = make_int2(0, 0);
        if (is_long) a.split_cur[int64_t(m) * a.maxL] = 0;
        a.lvl_cur[m] = offered ? Level{1, nch, is_long ? 1 : 0, 0} : Level{0, 0, 0, 0};
        a.root[m * 4] = 0; a.root[m * 4 + 1] = 0; a.root[m * 4 + 2] = 0;
    }
}

// ------------------------------------------------------------------------------------------------------ a level
using gae::cells::Lds;
using gae::cells::Node;

// work item `item` of model m's level: its node as the level pass sees it
__device__ __forceinline__ Node node_of(const Args &a, int m, int item)
{
    const Item it = a.items_cur[int64_t(m) * a.maxI + item];
    return Node{int64_t(m) * a.M + it.node, int64_t(m) * a.n_used, int64_t(m) * a.maxI + item,
                it.slot >= 0 ? int64_t(m) * a.maxL + it.slot : -1, it.node,
                (uint64_t(1) << 32) + ((uint64_t(a.round) << 8) | uint64_t(m % (a.folds + 1)))};
}

// a cell holds two sums: the model's fixed-point g and h of the listed rows
struct GradHess {
    const i64 *gq, *hq;
    __device__ GradHess(const Args &a, int m) : gq(a.gq + int64_t(m) * a.n_used), hq(a.hq + int64_t(m) * a.n_used) {}
    __device__ constexpr int words() const { return 2; }
    __device__ i64 word(int s, int j) const { return j == 0 ? gq[s] : hq[s]; }
};

// the score of a split of node `at` of model m: G_l^2 / (H_l + lambda) + G_r^2 / (H_r + lambda), under min_child_weight
struct Gain {
    const Args &a;
    i64 G, H;
    double lam;
    __device__ Gain(const Args &a_, int m, int64_t at) : a(a_), G(a_.nG[at]), H(a_.nH[at]), lam(a_.lam[m / (a_.folds + 1)]) {}
    __device__ constexpr int words() const { return 2; }
    __device__ double score(const Lds &h, int idx, int, int) const
    {
        const i64 glq = h.sum[idx * 2], hlq = h.sum[idx * 2 + 1];
        const double gl = double(glq) * a.g_step, gr = double(G - glq) * a.g_step;
        const double hl = double(hlq) * a.h_step, hr = double(H - hlq) * a.h_step;
        if (!(hl >= a.mcw) || !(hr >= a.mcw)) return -1.0;
        const double dl = hl + lam, dr = hr + lam;
        if (!(dl > 0.0) || !(dr > 0.0)) return -1.0;
        const double score = (gl * gl) / dl + (gr * gr) / dr;
        return score;
    }
};

// grid models . gx, gx = chunk bound . nft: block b of a model is tile b % nft of its chunk b / nft
__global__ __launch_bounds__(kThreads) void boost_hist_kernel(const Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int m = blockIdx.x / a.gx, bx = blockIdx.x % a.gx, c = bx / a.nft, tile = bx % a.nft;
    if (c >= a.lvl_cur[m].n_chunks) return;
    const Lds h = gae::cells::carve(lds, a.ft, a.bins, 2);
    const Chunk ch = a.chunks_cur[int64_t(m) * a.maxC + c];
    const Node nd = node_of(a, m, ch.item);
    if (gae::cells::fill_tile(a, h, GradHess(a, m), nd, ch, tile)) return;  // a node of several chunks: scanned later
    gae::cells::scan_tile(a, h, Gain(a, m, nd.at), nd, tile);
}

// grid models . gl, gl = long-node bound . nft: the merged cells of a long node; the slot is left zeroed for the next level
__global__ __launch_bounds__(kThreads) void boost_scan_kernel(const Args a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int m = blockIdx.x / a.gl, bx = blockIdx.x % a.gl, slot = bx / a.nft, tile = bx % a.nft;
    if (slot >= a.lvl_cur[m].n_long) return;
    const Lds h = gae::cells::carve(lds, a.ft, a.bins, 2);
    const Node nd = node_of(a, m, a.split_cur[int64_t(m) * a.maxL + slot]);
    gae::cells::load_slot<true>(a, h, 2, nd, int64_t(m) * a.maxL + slot, tile);
    gae::cells::scan_tile(a, h, Gain(a, m, nd.at), nd, tile);
}

// one block per model; a level holds at most 2^(depth - 1) <= 128 items: one per thread
__global__ __launch_bounds__(kThreads) void boost_decide_kernel(const Args a)
{
    __shared__ int w[kWaves];
    const int m = blockIdx.x, tid = threadIdx.x, cfg = m / (a.folds + 1);
    const Level lv = a.lvl_cur[m];
    const int base = a.n_nodes[m];
    const bool deeper = a.level + 1 < a.depth;
    const double lam = a.lam[cfg], lr = a.lr[cfg];
    int split = 0, bf = -1, bb = -1, n = 0;
    int64_t at = 0, cbest = 0;
    double best = -1.0, parent = 0.0;
    if (tid < lv.n_items) {
        const int64_t item = int64_t(m) * a.maxI + tid;
        at = int64_t(m) * a.M + a.items_cur[item].node;
        n = a.count[at];
        for (int tile = 0; tile < a.nft; ++tile) {         // tiles ascend in f: a strict > keeps the lower feature
            const int64_t c = item * a.nft + tile;
            const int2 fb = a.cand_fb[c];
            if (fb.x >= 0 && a.cand_score[c] > best) { best = a.cand_score[c]; bf = fb.x; bb = fb.y; cbest = c; }
        }
        const double g = double(a.nG[at]) * a.g_step, den = double(a.nH[at]) * a.h_step + lam;
        parent = den > 0.0 ? (g * g) / den : 0.0;
        split = (bf >= 0 && best > parent + a.min_gain) ? 1 : 0;
    }
    int total;
    const int k = block_scan(split, w, total);
    const int L = base + 2 * k;
    int nl = 0, wl = 0, wr = 0;
    if (split) {
        nl = a.cand_nl[cbest];
        if (L + 1 >= a.M || nl <= 0 || nl >= n) {
            flag(a.status, GAE_FOREST_ERR_NODE);           // cannot happen: the capacity bounds a binary tree
            split = 0;
        } else {
            a.feature[at] = bf; a.bin[at] = bb; a.left[at] = L;
            a.threshold[at] = a.edges[int64_t(bf) * (a.bins - 1) + bb];
            a.gain[at] = best - parent;
            const int64_t lt = int64_t(m) * a.M + L, rt = lt + 1;
            const int start = a.seg_start[at];
            const i64 gl = a.cand_sum[cbest * 2], hl = a.cand_sum[cbest * 2 + 1];
            const i64 gr = a.nG[at] - gl, hr = a.nH[at] - hl;
            a.count[lt] = nl; a.count[rt] = n - nl;
            a.seg_start[lt] = start; a.seg_start[rt] = start + nl;
            a.nG[lt] = gl; a.nH[lt] = hl; a.nG[rt] = gr; a.nH[rt] = hr;
            a.value[lt] = leaf_weight(a, gl, hl, lr, lam);
            a.value[rt] = leaf_weight(a, gr, hr, lr, lam);
            wl = (deeper && nl >= 2 * a.msl) ? 1 : 0;
            wr = (deeper && n - nl >= 2 * a.msl) ? 1 : 0;
        }
    }
    const int cl = wl ? chunks_of(nl) : 0, cr = wr ? chunks_of(n - nl) : 0;
    const int ll = (wl && nl > kSplitRows) ? 1 : 0, lr_ = (wr && n - nl > kSplitRows) ? 1 : 0;
    int tw, tc, tl;
    const int kw = block_scan(wl + wr, w, tw), kc = block_scan(cl + cr, w, tc), kl = block_scan(ll + lr_, w, tl);
    if (tw > a.maxI || tc > a.maxC || tl > a.maxL) {       // cannot happen: the bounds of the K30 comment
        if (tid == 0) {
            flag(a.status, GAE_FOREST_ERR_NODE);
            a.lvl_next[m] = Level{0, 0, 0, 0};
            a.n_nodes[m] = base + 2 * total;
        }
        return;
    }
    for (int q = 0; q < 2; ++q) {
        if (!(q ? wr : wl)) continue;
        const int item = kw + (q ? wl : 0), nch = q ? cr : cl;
        const int slot = (q ? lr_ : ll) ? kl + (q ? ll : 0) : -1;
        a.items_next[int64_t(m) * a.maxI + item] = Item{L + q, slot};
        a.curs_next[int64_t(m) * a.maxI + item] = make_int2(0, 0);
        if (slot >= 0) a.split_next[int64_t(m) * a.maxL + slot] = item;
        Chunk *out = a.chunks_next + int64_t(m) * a.maxC + kc + (q ? cl : 0);
        for (int c = 0; c < nch; ++c) out[c] = Chunk{item, c};
    }
    if (tid == 0) {
        a.lvl_next[m] = Level{tw, tc, tl, 0};
        a.n_nodes[m] = base + 2 * total;
    }
}

// grid (chunk bound, models)
__global__ __launch_bounds__(kThreads) void boost_partition_kernel(const Args a)
{
    const int m = blockIdx.y;
    if (int(blockIdx.x) >= a.lvl_cur[m].n_chunks) return;
    const Chunk ch = a.chunks_cur[int64_t(m) * a.maxC + blockIdx.x];
    gae::cells::partition_chunk(a, node_of(a, m, ch.item), ch.chunk);
}

// one block per configuration: the all-rows model's table of this round to the output
__global__ __launch_bounds__(kThreads) void boost_keep_kernel(const Args a)
{
    const int cfg = blockIdx.x, m = cfg * (a.folds + 1) + a.folds;
    const int64_t src = int64_t(m) * a.M, dst = (int64_t(cfg) * a.R + a.round) * a.M;
    for (int j = threadIdx.x; j < a.M; j += kThreads) {
        a.o_feature[dst + j] = a.feature[src + j]; a.o_bin[dst + j] = a.bin[src + j]; a.o_left[dst + j] = a.left[src + j];
        a.o_count[dst + j] = a.count[src + j]; a.o_threshold[dst + j] = a.threshold[src + j];
        a.o_value[dst + j] = a.value[src + j]; a.o_gain[dst + j] = a.gain[src + j];
    }
    if (threadIdx.x == 0) a.o_n_nodes[int64_t(cfg) * a.R + a.round] = a.n_nodes[m];
}

// ------------------------------------------------------------------------------------------------------ predict
struct PredictArgs {
    const float *X;
    int64_t ldx;
    int m, d, R, M;
    const int32_t *feature, *left;
    const float *threshold;
    const double *value;
    double base;
    double *out;
    gae_forest_status *status;
};

__global__ __launch_bounds__(kThreads) void boost_predict_kernel(const PredictArgs a)
{
    const int64_t row = int64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (row >= a.m) return;
    const float *x = a.X + row * a.ldx;
    bool finite = true;
    for (int f = 0; f < a.d; ++f) finite = finite && (fabsf(x[f]) <= FLT_MAX);
    double acc = a.base;
    bool broken = false;
    if (finite) {
        for (int r = 0; r < a.R && !broken; ++r) {
            const int64_t t0 = int64_t(r) * a.M;
            const int node = gae::cells::walk(a.feature + t0, a.left + t0, a.threshold + t0, x, a.d, a.M, kMaxDepth);
            if (node < 0) broken = true;
            else acc = acc + a.value[t0 + node];
        }
    } else {
        atomicAdd(reinterpret_cast<u64 *>(&a.status->nonfinite), u64(1));
    }
    if (broken) flag(a.status, GAE_FOREST_ERR_NODE);
    a.out[row] = (finite && !broken) ? acc : __builtin_nan("");
}

// ------------------------------------------------------------------------------------------------------ host
struct Plan {
    int64_t Mo, M, maxI, maxC, maxL, ft, nft, n_parts, need;
    int32_t *pos[2], *split[2];                             // the ping-pong halves of the level lists
    Item *items[2];
    Chunk *chunks[2];
    int2 *curs[2];
    Level *lvl[2];
    double *cfg;                                            // lr [n_cfg], lambda [n_cfg]
};

// the checks, the sizes and THE workspace layout: on ws = NULL the regions are only counted (p.need), on the caller's buffer
// they are bound into `a` and the halves of `p`
int plan(const char *fn, int64_t n_used, int64_t d, int64_t bins, int64_t depth, int64_t folds, int64_t n_cfg, void *ws, Plan &p,
         Args &a)
{
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..256", fn, (long long)d);
    GAE_REQUIRE(bins >= 2 && bins <= kMaxBins, GAE_E_RANGE, "%s: max_bins = %lld outside 2..256", fn, (long long)bins);
    GAE_REQUIRE(depth >= 1 && depth <= kMaxDepth, GAE_E_RANGE, "%s: max_depth = %lld outside 1..8", fn, (long long)depth);
    GAE_REQUIRE(folds == 0 || (folds >= 2 && folds < kMaxModels), GAE_E_RANGE, "%s: folds = %lld: 0 (no held-out models) or 2..255",
                fn, (long long)folds);
    GAE_REQUIRE(n_cfg >= 1 && n_cfg <= kMaxModels && (folds + 1) * n_cfg <= kMaxModels, GAE_E_RANGE,
                "%s: (folds + 1) n_cfg = %lld models outside 1..256", fn, (long long)((folds + 1) * n_cfg));
    GAE_REQUIRE(n_used >= 1 && n_used < (int64_t(1) << 31), GAE_E_SIZE, "%s: n_used = %lld outside 1..2^31", fn, (long long)n_used);
    p.Mo = (folds + 1) * n_cfg;
    p.M = (int64_t(1) << (depth + 1)) - 1;
    p.maxI = int64_t(1) << (depth - 1);
    p.maxC = p.maxI + cdiv(n_used, kSplitRows);
    p.maxL = n_used / kSplitRows;
    p.ft = gae::cells::tile_features(d, bins, 2);
    p.nft = cdiv(d, p.ft);
    p.n_parts = cdiv(n_used, kLossRows);
    GAE_REQUIRE(p.Mo * p.maxC * p.nft < (int64_t(1) << 31) && p.Mo * n_used < (int64_t(1) << 40), GAE_E_SIZE,
                "%s: %lld models of %lld rows are beyond the grids and lists", fn, (long long)p.Mo, (long long)n_used);
    const int64_t Mo = p.Mo, nodes = Mo * p.M, lmax = p.maxL > 0 ? p.maxL : 1;
    gae::Carver c(ws);
    p.cfg = c.take<double>(2 * n_cfg);
    a.feature = c.take<int32_t>(nodes); a.bin = c.take<int32_t>(nodes); a.left = c.take<int32_t>(nodes);
    a.count = c.take<int32_t>(nodes); a.seg_start = c.take<int32_t>(nodes); a.n_nodes = c.take<int32_t>(Mo);
    a.threshold = c.take<float>(nodes); a.value = c.take<double>(nodes); a.gain = c.take<double>(nodes);
    a.nG = c.take<i64>(nodes); a.nH = c.take<i64>(nodes);
    a.gq = c.take<i64>(Mo * n_used); a.hq = c.take<i64>(Mo * n_used);
    a.root = c.take<i64>(Mo * 4);
    take_halves(c, p.pos, Mo * n_used);
    take_halves(c, p.items, Mo * p.maxI);
    take_halves(c, p.chunks, Mo * p.maxC);
    take_halves(c, p.split, Mo * lmax);
    take_halves(c, p.curs, Mo * p.maxI);
    take_halves(c, p.lvl, Mo);
    a.cand_score = c.take<double>(Mo * p.maxI * p.nft);
    a.cand_fb = c.take<int2>(Mo * p.maxI * p.nft);
    a.cand_nl = c.take<int32_t>(Mo * p.maxI * p.nft);
    a.cand_sum = c.take<i64>(Mo * p.maxI * p.nft * 2);
    a.gcnt = c.take<unsigned>(Mo * lmax * d * bins);
    a.gsum = c.take<i64>(Mo * lmax * d * bins * 2);
    a.part = c.take<double>(Mo * p.n_parts);
    p.need = c.bytes() + 256;
    return GAE_OK;
}

} // namespace

extern "C" int64_t gae_boost_workspace_bytes(int64_t n_used, int64_t d, int64_t max_bins, int64_t max_depth, int64_t folds,
                                             int64_t n_cfg)
{
    Plan p;
    Args a;
    if (const int rc = plan("gae_boost_workspace_bytes", n_used, d, max_bins, max_depth, folds, n_cfg, nullptr, p, a)) return rc;
    return p.need;
}

extern "C" int gae_boost_fit(const uint8_t *codes, const int32_t *n_edges, const float *edges, int64_t n_used, int64_t d,
                             int64_t max_bins, const float *y, const int32_t *fold, int64_t folds, int objective,
                             double base_score, int32_t exponent, const double *learning_rates, const double *lambdas,
                             int64_t n_cfg, int64_t n_rounds, int64_t max_depth, int64_t max_features,
                             int64_t min_samples_leaf, double min_child_weight, double min_gain, uint64_t seed,
                             int64_t check_every, int32_t *feature, int32_t *threshold_bin, float *threshold, int32_t *left,
                             int32_t *count, double *value, double *gain, int32_t *n_nodes, double *loss, int64_t *correct,
                             double *score, int32_t *bad, gae_forest_status *status, void *workspace, int64_t workspace_bytes,
                             void *stream)
{
    const char *fn = "gae_boost_fit";
    Plan p;
    Args a;
    if (const int rc = plan(fn, n_used, d, max_bins, max_depth, folds, n_cfg, workspace, p, a)) return rc;
    GAE_REQUIRE(objective == GAE_BOOST_SQUARED || objective == GAE_BOOST_LOGISTIC, GAE_E_RANGE, "%s: unknown objective %d", fn,
                objective);
    GAE_REQUIRE(n_rounds >= 1 && n_rounds <= kMaxRounds, GAE_E_RANGE, "%s: n_rounds = %lld outside 1..4096", fn, (long long)n_rounds);
    GAE_REQUIRE(max_features >= 1 && max_features <= d, GAE_E_RANGE, "%s: max_features = %lld outside 1..d = %lld", fn,
                (long long)max_features, (long long)d);
    GAE_REQUIRE(min_samples_leaf >= 1 && min_samples_leaf < (int64_t(1) << 30), GAE_E_RANGE,
                "%s: min_samples_leaf = %lld outside 1..2^30", fn, (long long)min_samples_leaf);
    GAE_REQUIRE(check_every >= 1, GAE_E_RANGE, "%s: check_every = %lld < 1", fn, (long long)check_every);
    GAE_REQUIRE(min_child_weight >= 0.0 && min_child_weight <= DBL_MAX && min_gain >= 0.0 && min_gain <= DBL_MAX, GAE_E_RANGE,
                "%s: min_child_weight = %g, min_gain = %g: finite values >= 0", fn, min_child_weight, min_gain);
    GAE_REQUIRE(fabs(base_score) <= DBL_MAX && exponent >= -200 && exponent <= 200, GAE_E_RANGE,
                "%s: a non-finite base_score or exponent = %d outside -200..200", fn, exponent);
    GAE_REQUIRE(learning_rates && lambdas, GAE_E_NULL, "%s: learning_rates / lambdas is NULL", fn);
    for (int64_t c = 0; c < n_cfg; ++c) {
        GAE_REQUIRE(learning_rates[c] > 0.0 && learning_rates[c] <= 1.0, GAE_E_RANGE, "%s: learning_rates[%lld] = %g outside (0, 1]",
                    fn, (long long)c, learning_rates[c]);
        GAE_REQUIRE(lambdas[c] >= 0.0 && lambdas[c] <= DBL_MAX, GAE_E_RANGE, "%s: lambdas[%lld] = %g: a finite value >= 0", fn,
                    (long long)c, lambdas[c]);
        GAE_REQUIRE(min_child_weight > 0.0 || lambdas[c] > 0.0, GAE_E_RANGE,
                    "%s: min_child_weight = 0 with lambdas[%lld] = 0: a leaf could divide by zero", fn, (long long)c);
    }
    GAE_REQUIRE(codes && n_edges && edges && y, GAE_E_NULL, "%s: codes / n_edges / edges / y is NULL", fn);
    GAE_REQUIRE(folds == 0 || fold, GAE_E_NULL, "%s: fold is NULL with folds = %lld", fn, (long long)folds);
    GAE_REQUIRE(feature && threshold_bin && threshold && left && count && value && gain && n_nodes && loss && correct && score &&
                    bad && status,
                GAE_E_NULL, "%s: an output or status is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(workspace_bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)p.need);

    a.codes = codes; a.n_edges = n_edges; a.edges = edges; a.y = y; a.fold = fold;
    a.n_used = int(n_used); a.d = int(d); a.bins = int(max_bins); a.folds = int(folds); a.n_cfg = int(n_cfg); a.Mo = int(p.Mo);
    a.depth = int(max_depth); a.M = int(p.M); a.m_feat = int(max_features); a.msl = int(min_samples_leaf);
    a.objective = objective; a.R = int(n_rounds); a.ft = int(p.ft); a.nft = int(p.nft); a.maxI = int(p.maxI);
    a.maxC = int(p.maxC); a.maxL = int(p.maxL); a.n_parts = int(p.n_parts); a.round = 0; a.level = 0; a.gx = 1; a.gl = 1;
    a.mcw = min_child_weight; a.min_gain = min_gain; a.base = base_score;
    const int e = objective == GAE_BOOST_LOGISTIC ? 30 : exponent;
    a.g_up = ldexp(1.0, e); a.g_step = ldexp(1.0, -e);
    a.h_up = objective == GAE_BOOST_LOGISTIC ? ldexp(1.0, 30) : 1.0;
    a.h_step = objective == GAE_BOOST_LOGISTIC ? ldexp(1.0, -30) : 1.0;
    a.key = seed ^ GAE_FOREST_KEY_XOR;
    a.lr = p.cfg; a.lam = p.cfg + n_cfg;
    a.o_feature = feature; a.o_bin = threshold_bin; a.o_left = left; a.o_count = count; a.o_n_nodes = n_nodes;
    a.o_threshold = threshold; a.o_value = value; a.o_gain = gain; a.loss = loss; a.score = score; a.correct = reinterpret_cast<i64 *>(correct);
    a.bad = bad; a.status = status;
    auto side = [&](int cur) {
        a.pos_in = p.pos[cur]; a.pos_out = p.pos[cur ^ 1];
        a.items_cur = p.items[cur]; a.items_next = p.items[cur ^ 1];
        a.chunks_cur = p.chunks[cur]; a.chunks_next = p.chunks[cur ^ 1];
        a.split_cur = p.split[cur]; a.split_next = p.split[cur ^ 1];
        a.curs = p.curs[cur]; a.curs_next = p.curs[cur ^ 1];
        a.lvl_cur = p.lvl[cur]; a.lvl_next = p.lvl[cur ^ 1];
    };
    hipStream_t st = gae::as_stream(stream);
    const int64_t Mo = p.Mo, lmax = p.maxL > 0 ? p.maxL : 1;

    GAE_HIP(hipMemcpyAsync(p.cfg, learning_rates, size_t(n_cfg) * 8, hipMemcpyHostToDevice, st));
    GAE_HIP(hipMemcpyAsync(p.cfg + n_cfg, lambdas, size_t(n_cfg) * 8, hipMemcpyHostToDevice, st));
    GAE_HIP(hipMemsetAsync(a.root, 0, size_t(Mo) * 4 * 8, st));
    GAE_HIP(hipMemsetAsync(a.gcnt, 0, size_t(Mo) * lmax * d * max_bins * 4, st));
    GAE_HIP(hipMemsetAsync(a.gsum, 0, size_t(Mo) * lmax * d * max_bins * 16, st));
    GAE_HIP(hipMemsetAsync(bad, 0, size_t(Mo) * 4, st));
    GAE_HIP(hipMemsetAsync(correct, 0, size_t(Mo) * (n_rounds + 1) * 8, st));

    const size_t lds = gae::cells::lds_bytes(int(p.ft), int(max_bins), 2);
    const dim3 block(kThreads);
    auto head = [&](int round) -> int {
        a.round = round;
        side(0);
        hipLaunchKernelGGL(boost_prologue_kernel, dim3(unsigned(p.n_parts), unsigned(Mo)), block, 0, st, a);
        GAE_CHECK_LAUNCH("boost_prologue_kernel");
        hipLaunchKernelGGL(boost_root_kernel, dim3(unsigned(Mo)), block, 0, st, a);
        GAE_CHECK_LAUNCH("boost_root_kernel");
        return GAE_OK;
    };
    gae_forest_status seen = {0, 0, {0, 0}};
    for (int round = 0; round < n_rounds; ++round) {
        if (const int rc = head(round)) return rc;
        int cur = 0;
        for (int level = 0; level < max_depth; ++level) {
            a.level = level;
            side(cur);
            const int64_t items = std::min<int64_t>(int64_t(1) << level, p.maxI);
            const int64_t chunks = std::min<int64_t>(items + cdiv(n_used, kSplitRows), p.maxC);
            const int64_t longs = std::min<int64_t>(items, p.maxL);
            a.gx = int(chunks * p.nft); a.gl = int(longs * p.nft);
            if (const int rc = gae::launch_lds<&boost_hist_kernel>("boost_hist_kernel", Mo * a.gx, kThreads, lds, st, a))
                return rc;
            if (longs > 0)
                if (const int rc = gae::launch_lds<&boost_scan_kernel>("boost_scan_kernel", Mo * a.gl, kThreads, lds, st, a))
                    return rc;
            hipLaunchKernelGGL(boost_decide_kernel, dim3(unsigned(Mo)), block, 0, st, a);
            GAE_CHECK_LAUNCH("boost_decide_kernel");
            if (level + 1 >= max_depth) break;             // the children are leaves: no lists, no partition
            hipLaunchKernelGGL(boost_partition_kernel, dim3(unsigned(chunks), unsigned(Mo)), block, 0, st, a);
            GAE_CHECK_LAUNCH("boost_partition_kernel");
            cur ^= 1;
        }
        hipLaunchKernelGGL(boost_keep_kernel, dim3(unsigned(n_cfg)), block, 0, st, a);
        GAE_CHECK_LAUNCH("boost_keep_kernel");
        if ((round + 1) % check_every == 0 && round + 1 < n_rounds) {
            GAE_HIP(hipMemcpyAsync(&seen, status, sizeof(seen), hipMemcpyDeviceToHost, st));
            GAE_HIP(hipStreamSynchronize(st));
            if (seen.errors || seen.nonfinite || seen.reserved[0] >= Mo) return GAE_OK;    // the caller reads the status and raises
        }
    }
    if (const int rc = head(int(n_rounds))) return rc;
    return GAE_OK;
}

extern "C" int gae_boost_predict(const float *X, int64_t ldx, int64_t m, int64_t d, int64_t n_rounds, int64_t node_capacity,
                                 const int32_t *feature, const float *threshold, const int32_t *left, const double *value,
                                 double base_score, double *out, gae_forest_status *status, void *stream)
{
    const char *fn = "gae_boost_predict";
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..256", fn, (long long)d);
    GAE_REQUIRE(n_rounds >= 0 && n_rounds <= kMaxRounds, GAE_E_RANGE, "%s: n_rounds = %lld outside 0..4096", fn, (long long)n_rounds);
    GAE_REQUIRE(m >= 0 && m < (int64_t(1) << 31), GAE_E_SIZE, "%s: m = %lld outside 0..2^31", fn, (long long)m);
    GAE_REQUIRE(node_capacity >= 1 && node_capacity <= 511, GAE_E_SIZE, "%s: node_capacity = %lld outside 1..511", fn,
                (long long)node_capacity);
    GAE_REQUIRE(ldx >= d, GAE_E_SIZE, "%s: ldx = %lld < d = %lld", fn, (long long)ldx, (long long)d);
    GAE_REQUIRE(status && (n_rounds == 0 || (feature && threshold && left && value)), GAE_E_NULL,
                "%s: a node table or status is NULL", fn);
    GAE_REQUIRE(m == 0 || (X && out), GAE_E_NULL, "%s: X / out is NULL", fn);
    if (m == 0) return GAE_OK;
    const PredictArgs a{X, ldx, int(m), int(d), int(n_rounds), int(node_capacity), feature, left, threshold, value, base_score,
                        out, status};
    hipLaunchKernelGGL(boost_predict_kernel, dim3(unsigned(cdiv(m, kThreads))), dim3(kThreads), 0, gae::as_stream(stream), a);
    GAE_CHECK_LAUNCH("boost_predict_kernel");
    return GAE_OK;
}
