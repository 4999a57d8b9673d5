// What the heads that work from fp64 moments share on the device (K25 ridge.hip, K28 logreg.hip, K31 pca.hip, K32
// spectral.hip): the walk over a row list cut into folds and chunks, the row-id fetch, the deal of the upper-triangle
// tiles of a Gram matrix, and the launch body that adds the chunk partials of a list of entries.
#pragma once
#include "common.h"

namespace gae {

typedef double v4d __attribute__((ext_vector_type(4)));

// n_rows listed rows in F folds: fold f is rows[fold_ptr[f] .. fold_ptr[f + 1]).  rows == NULL: the rows 0 .. n_rows - 1
// themselves, one fold, fold_ptr not read.
struct FoldList {
    const int32_t *rows, *fold_ptr;
    int F, n_rows;
};

// 0 <= fold_ptr[0] <= ... <= fold_ptr[F] == n_rows
__device__ __forceinline__ bool folds_valid(const FoldList &l)
{
    if (!l.rows) return true;
    int prev = l.fold_ptr[0];
    bool ok = prev >= 0;
    for (int f = 1; f <= l.F; ++f) {
        const int v = l.fold_ptr[f];
        ok = ok && v >= prev;
        prev = v;
    }
    return ok && prev == l.n_rows;
}

// the chunks (of chunk_rows rows, the last one shorter) of fold f
__device__ __forceinline__ int64_t fold_chunks(const FoldList &l, int f, int chunk_rows, int &lo, int &hi)
{
    if (l.rows) { lo = l.fold_ptr[f]; hi = l.fold_ptr[f + 1]; }
    else { lo = 0; hi = l.n_rows; }
    return (int64_t(hi) - lo + chunk_rows - 1) / chunk_rows;
}

// THE chunk order: folds ascending, chunks inside a fold ascending; a chunk never straddles folds.  Chunk b is the list
// positions lo .. hi - 1 of `fold`; fold < 0: b lies past the last chunk (a grid sized by an upper bound has spare blocks)
struct Chunk {
    int fold, lo, hi;
};

__device__ __forceinline__ Chunk chunk_of(const FoldList &l, int64_t b, int chunk_rows)
{
    for (int f = 0; f < l.F; ++f) {
        int flo, fhi;
        const int64_t nc = fold_chunks(l, f, chunk_rows, flo, fhi);
        if (b < nc) {
            const int lo = int(flo + b * chunk_rows);
            return Chunk{f, lo, fhi - lo > chunk_rows ? lo + chunk_rows : fhi};
        }
        b -= nc;
    }
    return Chunk{-1, 0, 0};
}

// the index of fold f's first chunk
__device__ __forceinline__ int64_t chunks_before(const FoldList &l, int f, int chunk_rows)
{
    int64_t base = 0;
    int lo, hi;
    for (int g = 0; g < f; ++g) base += fold_chunks(l, g, chunk_rows, lo, hi);
    return base;
}

// the row id at list position i, or -1 (and bad = true) when it lies outside [0, n)
__device__ __forceinline__ int row_id(const FoldList &l, int64_t i, int n, bool &bad)
{
    const int id = l.rows ? l.rows[i] : int(i);
    if (unsigned(id) >= unsigned(n)) { bad = true; return -1; }
    return id;
}

// ---- the upper triangle of a symmetric product in tiles of 16: NT (NT + 1) / 2 tiles in row order; e -> (ti, tj), ti <= tj
__device__ __forceinline__ void upper_tile(int e, int NT, int &ti, int &tj)
{
    int r = 0;
    while (e >= NT - r) { e -= NT - r; ++r; }
    ti = r; tj = r + e;
}
// the LDS pitch (in fp64) of a staged row of NT tiles: pitch / 16 odd, so the four rows of a v_mfma_f64_16x16x4_f64 operand
// start 32 banks apart
constexpr int tile_pitch(int NT) { return (NT & 1) ? 16 * NT : 16 * NT + 16; }

// ---- the body of a launch of kThreads-thread blocks that adds the P chunk partials part[q E + e], q ascending, of the
// entries e < E with keep(e), in THE order of partial lists (common.h), and hands each sum to put(e, sum).  P <= 32: one
// thread per entry, ceil(E / kThreads) blocks do the work; more: one wave per kWaveEntries entries (P may be known on
// the device only: a grid of ceil(E / (kThreads / 64 . kWaveEntries)) blocks covers both)
constexpr int kWaveEntries = 4;

template <int kThreads, class Keep, class Put>
__device__ __forceinline__ void reduce_entries(const double *__restrict__ part, int64_t P, int64_t E, Keep keep, Put put)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (partial_lanes(P) == 1) {
        const int64_t e = int64_t(blockIdx.x) * kThreads + tid;
        if (e < E && keep(e)) put(e, sum_partials(part + e, P, E, 0, 1));
    } else {
#pragma unroll
        for (int i = 0; i < kWaveEntries; ++i) {                       // all 64 lanes of the wave call
            const int64_t e = (int64_t(blockIdx.x) * (kThreads / kWave) + wave) * kWaveEntries + i;
            if (e >= E) break;
            if (!keep(e)) continue;
            const double s = sum_partials(part + e, P, E, lane, 64);
            if (lane == 0) put(e, s);
        }
    }
}

} // namespace gae
