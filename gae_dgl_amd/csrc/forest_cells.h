// What the histogram-tree families share (K26 forest.hip, K30 boost.hip): the block scan of the level kernels, the Philox
// feature-subset rule, the order of two candidates and the carve of one feature tile's LDS cells.  Blocks of 256 threads.
#pragma once
#include "common.h"

namespace gae {
namespace cells {

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kHistBytes = 64 * 1024;      // LDS cells of one feature tile

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

} // namespace cells
} // namespace gae
