// K17: unbiased sampled estimate of the fused decoder + weighted BCE loss (gae_decoder_bce_sampled).
//
// The reference's loss (train_inductive.py:44-48) splits exactly into an all-pairs term and an edge term:
//   L = (1/N^2) [ sum_{all i,j} sp(x_ij) + sum_{edges e=(i,j)} (pw sp(-x_e) - sp(x_e)) ],  sp = softplus,
// so only the all-pairs sum needs sampling, and sampling it uniformly needs no edge-membership test.  Per local row r
// the estimate takes m distinct partners pi_s(r), s < m, from a keyed bijection (the sampler below) and weights them
// N / m; the edge sum is exact.  E[estimate] = L; at m = N every pair appears once and the estimate is L.
//
// Work: every local row r owns ONE ordered pair list
//   [ its edges (CSR of A) | its transposed edges (CSR of A^T, gradient only) | its m samples | its m inverse partners
//     (gradient only) ]
// and its gradient row is the sum over that list, in that order.  A wave walks the list P = 64 / G pairs at a time
// (G = d/4 lanes per pair, 16-byte loads of Zt), reduces each dot product over its lane group, evaluates softplus /
// sigmoid once per pair and FMAs the coefficient times the partner row into the lane's accumulator.  Rows whose list is
// longer than CH (4096 pairs at level 0) are "heavy": they are cut into chunks of CH pairs that any wave of a
// persistent launch evaluates, and a second pass adds the chunk partials in chunk order.  Which rows are heavy and where
// the chunk boundaries lie depend only on the row, so dZ has the same bits whatever the grid or the row partition (the
// one exception: graphs whose heavy rows hold more pairs than the chunk store -- n_local / 16 + 1024 chunks -- has room
// for at CH = 4096 use the smallest CH << level that fits; the level is the same for every partition in all practical
// cases).
//
// Launches: prepare + count, scan, place, rows, chunks, heavy rows, finalize.  Loss: fp64 partials per 16-row block and
// per heavy row, added in a fixed order by one block.
#include "common.h"

namespace {

constexpr int kTileRows = 256;       // rows per counting tile (one thread each)
constexpr int kBlockRows = 16;       // rows per block of the row kernel (4 waves x 4 rows)
constexpr int kLevels = 16;          // chunk sizes CH << level, level = 0 .. 15
constexpr int64_t kChunk = 4096;     // CH: pairs per chunk at level 0 (a multiple of 64)
constexpr int kPrepElems = 2048;     // Zt elements per block of the prepare step

constexpr uint64_t kSamplerKeyXor = 0xD1B54A32D192ED03ull;   // the sampler's Philox key = seed ^ this

struct SArgs {
    const float *Z;
    float *mask;
    int64_t ldz;
    int n, d, DP, m;
    int64_t row_begin;
    int n_local;
    const int32_t *indptr, *indices, *t_indptr, *t_indices;
    float pw, drop_p, drop_scale, inv_n2f;
    double inv_n2;
    uint64_t seed, offset;
    uint64_t *draw_dev;
    float *loss_out, *dZ;
    int64_t lddz;
    int32_t *partners_out;
    bool grad;
    // workspace
    float *Zt;
    int32_t *tile_cnt;        // [n_tiles][2][kLevels]: heavy rows, chunks
    int64_t *tile_base;       // [n_tiles][2]: first heavy slot, first chunk
    int64_t *hdr;             // level, chunks, heavy rows, overflow
    double *block_loss;       // [n_b3]
    int64_t *heavy;           // [cap][3]: local row, chunks, first chunk
    int32_t *chunk_slot;      // [cap]
    float *cpart;             // [cap][DP]
    double *closs, *hloss;    // [cap]
    int64_t cap;
    int n_tiles, n_b3;
};

// ---------------------------------------------------------------------------------------------------------------
// The sampler (documented bit for bit in include/gae_hip_experimental.h; tests/sampled_ref.py restates it in numpy)
// ---------------------------------------------------------------------------------------------------------------
struct Perm {
    uint32_t k[4];
    uint32_t n;
    int wl, wr;       // widths of the left / right part before round 0
};

__device__ __forceinline__ uint32_t round_fn(uint32_t r, uint32_t k)
{
    uint32_t x = r ^ k;
    x *= 0x9E3779B1u;
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    return x;
}

__device__ __forceinline__ uint32_t lowmask(int w) { return w >= 32 ? 0xffffffffu : (1u << w) - 1u; }

__device__ __forceinline__ uint32_t feistel_enc(const Perm &p, uint32_t v)
{
    int wl = p.wl, wr = p.wr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t L = wr >= 32 ? 0u : v >> wr, R = v & lowmask(wr);
        v = (wl >= 32 ? 0u : R << wl) | (L ^ (round_fn(R, p.k[r]) & lowmask(wl)));
        const int t = wl; wl = wr; wr = t;
    }
    return v;
}

__device__ __forceinline__ uint32_t feistel_dec(const Perm &p, uint32_t v)
{
#pragma unroll
    for (int r = 3; r >= 0; --r) {
        const int wl = (r & 1) ? p.wr : p.wl, wr = (r & 1) ? p.wl : p.wr;   // widths before round r
        const uint32_t R = wl >= 32 ? 0u : v >> wl, X = v & lowmask(wl);
        const uint32_t L = X ^ (round_fn(R, p.k[r]) & lowmask(wl));
        v = (wr >= 32 ? 0u : L << wr) | R;
    }
    return v;
}

// cycle walking: the bijection of [0, 2^b) restricted to [0, n) (expected < 2 rounds: 2^b < 2 n)
__device__ __forceinline__ uint32_t perm_fwd(const Perm &p, uint32_t i)
{
    uint32_t v = feistel_enc(p, i);
    while (v >= p.n) v = feistel_enc(p, v);
    return v;
}
__device__ __forceinline__ uint32_t perm_inv(const Perm &p, uint32_t y)
{
    uint32_t v = feistel_dec(p, y);
    while (v >= p.n) v = feistel_dec(p, v);
    return v;
}

// sigma (Philox block 0) and tau (block 1) of draw t
__device__ __forceinline__ void sampler_keys(uint64_t seed, uint64_t t, uint32_t n, Perm &sig, Perm &tau)
{
    int b = 0;
    while ((uint64_t(1) << b) < uint64_t(n)) ++b;
    const int h = b >> 1;
    uint32_t c[4];
    gae::philox4x32_10(0, t, seed ^ kSamplerKeyXor, c);
#pragma unroll
    for (int q = 0; q < 4; ++q) sig.k[q] = c[q];
    gae::philox4x32_10(1, t, seed ^ kSamplerKeyXor, c);
#pragma unroll
    for (int q = 0; q < 4; ++q) tau.k[q] = c[q];
    sig.n = tau.n = n;
    sig.wl = tau.wl = b - h;
    sig.wr = tau.wr = h;
}

__device__ __forceinline__ uint64_t draw_of(const SArgs &a) { return a.draw_dev ? *a.draw_dev : 0; }

__device__ __forceinline__ int64_t pair_count(const SArgs &a, int rl, int &deg, int &tdeg)
{
    deg = a.indptr[rl + 1] - a.indptr[rl];
    tdeg = a.grad ? a.t_indptr[rl + 1] - a.t_indptr[rl] : 0;
    return int64_t(deg) + tdeg + (a.grad ? 2 * int64_t(a.m) : int64_t(a.m));
}

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.f) + log1pf(__expf(-fabsf(x))); }

// ---------------------------------------------------------------------------------------------------------------
// One wave: pairs [p0, p1) of local row rl's list.  acc (lane's 4 columns, summed over its lane group's pairs) and
// lsum (fp64, lane sub == 0 only) are accumulated; the caller reduces over the groups.
// ---------------------------------------------------------------------------------------------------------------
template <int G>
__device__ __forceinline__ void process_pairs(const SArgs &a, const Perm &sig, const Perm &tau, int rl, int64_t p0,
                                              int64_t p1, int deg, int tdeg, uint32_t sig_r, const gae::v4f &zr,
                                              gae::v4f &acc, double &lsum)
{
    constexpr int P = 64 / G;
    const int lane = threadIdx.x & 63, grp = lane / G, sub = lane % G;
    const bool col_ok = sub * 4 < a.DP;
    const int32_t *row_idx = a.indices + a.indptr[rl];
    const int32_t *trow_idx = a.grad ? a.t_indices + a.t_indptr[rl] : nullptr;
    const uint32_t N = uint32_t(a.n);
    const float w = float(a.n) / float(a.m);
    for (int64_t base = p0; base < p1; base += P) {
        const int64_t p = base + grp;
        const bool valid = p < p1;
        int kind = 0;                   // 0 edge, 1 transposed edge, 2 sample, 3 inverse partner
        uint32_t j = 0;
        if (valid) {
            int64_t q = p;
            if (q < deg) {
                j = uint32_t(row_idx[q]);
            } else {
                q -= deg;
                if (q < tdeg) {
                    kind = 1; j = uint32_t(trow_idx[q]);
                } else {
                    q -= tdeg;
                    if (q < a.m) {
                        kind = 2;
                        const uint32_t o = perm_fwd(tau, uint32_t(q));
                        j = perm_inv(sig, uint32_t((uint64_t(sig_r) + o) % N));
                        if (sub == 0 && a.partners_out) a.partners_out[int64_t(rl) * a.m + q] = int32_t(j);
                    } else {
                        kind = 3;
                        const uint32_t o = perm_fwd(tau, uint32_t(q - a.m));
                        j = perm_inv(sig, uint32_t((uint64_t(sig_r) + N - o) % N));
                    }
                }
            }
        }
        gae::v4f zp = {0.f, 0.f, 0.f, 0.f};
        if (valid && col_ok) zp = *reinterpret_cast<const gae::v4f *>(a.Zt + int64_t(j) * a.DP + sub * 4);
        float x = zr[0] * zp[0];
        x = fmaf(zr[1], zp[1], x);
        x = fmaf(zr[2], zp[2], x);
        x = fmaf(zr[3], zp[3], x);
#pragma unroll
        for (int o = 1; o < G; o <<= 1) x += __shfl_xor(x, o, 64);
        float coef = 0.f;
        double term = 0.0;
        if (valid) {
            if (kind < 2) {
                // pw sp(-x) - sp(x);  d/dx = -pw sigmoid(-x) - sigmoid(x)
                const float e = __expf(-fabsf(x));
                const float sp_pos = fmaxf(x, 0.f) + log1pf(e), sp_neg = sp_pos - x;
                const float s_pos = 1.f / (1.f + __expf(-x)), s_neg = 1.f / (1.f + __expf(x));
                coef = -a.pw * s_neg - s_pos;
                if (kind == 0) term = double(a.pw) * double(sp_neg) - double(sp_pos);
            } else {
                // (N / m) sp(x);  d/dx = (N / m) sigmoid(x)
                coef = w * (1.f / (1.f + __expf(-x)));
                if (kind == 2) term = double(w) * double(softplus(x));
            }
        }
        acc[0] = fmaf(coef, zp[0], acc[0]);
        acc[1] = fmaf(coef, zp[1], acc[1]);
        acc[2] = fmaf(coef, zp[2], acc[2]);
        acc[3] = fmaf(coef, zp[3], acc[3]);
        if (sub == 0) lsum += term;
    }
}

template <int G>
__device__ __forceinline__ void reduce_groups(gae::v4f &acc)
{
#pragma unroll
    for (int o = G; o < 64; o <<= 1) {
        acc[0] += __shfl_xor(acc[0], o, 64); acc[1] += __shfl_xor(acc[1], o, 64);
        acc[2] += __shfl_xor(acc[2], o, 64); acc[3] += __shfl_xor(acc[3], o, 64);
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float mask_of(const SArgs &a, int64_t rg, int k)
{
    return a.mask ? a.mask[rg * a.ldz + k] : 1.f;
}

// ---------------------------------------------------------------------------------------------------------------
// 1. Zt = Z (.) mask (mask drawn here when drop_p > 0: the Philox stream of gae_dropout_mask at this draw), padded to
//    DP columns; per 256-row tile of the local rows: heavy rows and chunks at every level
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sampled_prep_count_kernel(SArgs a, int prep_blocks)
{
    const int tid = threadIdx.x;
    if (int(blockIdx.x) < prep_blocks) {
        const int64_t total = int64_t(a.n) * a.DP;
        const bool draw = a.drop_p > 0.f;
        const uint64_t draw_idx = (draw && a.draw_dev) ? *a.draw_dev : 0;
        const int64_t e0 = int64_t(blockIdx.x) * kPrepElems;
        for (int64_t e = e0 + tid; e < e0 + kPrepElems && e < total; e += 256) {
            const int64_t i = e / a.DP;
            const int k = int(e % a.DP);
            float v = 0.f;
            if (k < a.d) {
                v = a.Z[i * a.ldz + k];
                if (draw) {
                    const int64_t el = i * a.d + k;
                    uint32_t c[4];
                    gae::philox4x32_10(a.offset + uint64_t(el >> 2), draw_idx, a.seed, c);
                    const uint32_t bits = (el & 2) ? ((el & 1) ? c[3] : c[2]) : ((el & 1) ? c[1] : c[0]);
                    const float mk = gae::dropout_multiplier(bits, a.drop_p, a.drop_scale);
                    a.mask[i * a.ldz + k] = mk;
                    v *= mk;
                } else if (a.mask) {
                    v *= a.mask[i * a.ldz + k];
                }
            }
            a.Zt[e] = v;
        }
    }
    if (int(blockIdx.x) < a.n_tiles) {
        __shared__ int cnt[2 * kLevels];
        if (tid < 2 * kLevels) cnt[tid] = 0;
        __syncthreads();
        const int rl = int(blockIdx.x) * kTileRows + tid;
        if (rl < a.n_local) {
            int deg, tdeg;
            const int64_t L = pair_count(a, rl, deg, tdeg);
            for (int lev = 0; lev < kLevels; ++lev) {
                const int64_t ch = kChunk << lev;
                if (L > ch) {
                    atomicAdd(&cnt[lev], 1);                               // (integer: exact in any order)
                    atomicAdd(&cnt[kLevels + lev], int((L + ch - 1) / ch));
                }
            }
        }
        __syncthreads();
        if (tid < 2 * kLevels) a.tile_cnt[int64_t(blockIdx.x) * 2 * kLevels + tid] = cnt[tid];
    }
}

// 2. one block: the level (smallest chunk size whose chunks fit the store), tile bases of heavy slots and chunks
__global__ __launch_bounds__(1024) void sampled_scan_kernel(SArgs a)
{
    __shared__ unsigned long long tot[2 * kLevels];
    __shared__ int64_t seg[2][1024];
    __shared__ int level_s;
    const int tid = threadIdx.x;
    if (tid < 2 * kLevels) tot[tid] = 0;
    __syncthreads();
    for (int q = 0; q < 2 * kLevels; ++q) {
        unsigned long long s = 0;
        for (int t = tid; t < a.n_tiles; t += 1024) s += unsigned(a.tile_cnt[int64_t(t) * 2 * kLevels + q]);
        if (s) atomicAdd(&tot[q], s);                                      // (integer: exact in any order)
    }
    __syncthreads();
    if (tid == 0) {
        int lev = kLevels - 1;
        for (int l = 0; l < kLevels; ++l)
            if (int64_t(tot[kLevels + l]) <= a.cap) { lev = l; break; }
        level_s = lev;
        const int64_t chunks = int64_t(tot[kLevels + lev]);
        // overflow (needs > 2^36 pairs in heavy rows): no chunk is evaluated and the loss is NaN
        const bool over = chunks > a.cap;
        a.hdr[0] = lev;
        a.hdr[1] = over ? 0 : chunks;
        a.hdr[2] = over ? 0 : int64_t(tot[lev]);
        a.hdr[3] = over ? 1 : 0;
    }
    __syncthreads();
    const int lev = level_s;
    // contiguous segments of tiles per thread: segment sums, exclusive scan of the 1024 sums, then the tiles
    const int per = (a.n_tiles + 1023) / 1024;
    const int t0 = tid * per, t1 = min(a.n_tiles, t0 + per);
    int64_t sh = 0, sc = 0;
    for (int t = t0; t < t1; ++t) {
        sh += a.tile_cnt[int64_t(t) * 2 * kLevels + lev];
        sc += a.tile_cnt[int64_t(t) * 2 * kLevels + kLevels + lev];
    }
    seg[0][tid] = sh; seg[1][tid] = sc;
    __syncthreads();
    if (tid == 0) {
        int64_t rh = 0, rc = 0;
        for (int q = 0; q < 1024; ++q) {
            const int64_t h = seg[0][q], c = seg[1][q];
            seg[0][q] = rh; seg[1][q] = rc;
            rh += h; rc += c;
        }
    }
    __syncthreads();
    sh = seg[0][tid]; sc = seg[1][tid];
    for (int t = t0; t < t1; ++t) {
        a.tile_base[2 * int64_t(t)] = sh;
        a.tile_base[2 * int64_t(t) + 1] = sc;
        sh += a.tile_cnt[int64_t(t) * 2 * kLevels + lev];
        sc += a.tile_cnt[int64_t(t) * 2 * kLevels + kLevels + lev];
    }
}

// 3. heavy rows of a tile -> their slot (row order) and their chunks' descriptors
__global__ __launch_bounds__(256) void sampled_place_kernel(SArgs a)
{
    const int lev = int(a.hdr[0]);
    const int64_t t = blockIdx.x;
    if (a.tile_cnt[t * 2 * kLevels + lev] == 0) return;                   // (block-uniform)
    __shared__ int64_t hs[kTileRows], cs[kTileRows];
    const int tid = threadIdx.x;
    const int rl = int(t) * kTileRows + tid;
    const int64_t ch = kChunk << lev;
    int64_t L = 0;
    if (rl < a.n_local) {
        int deg, tdeg;
        L = pair_count(a, rl, deg, tdeg);
    }
    const bool heavy = L > ch;
    const int64_t nch = heavy ? (L + ch - 1) / ch : 0;
    hs[tid] = heavy ? 1 : 0; cs[tid] = nch;
    __syncthreads();
    if (tid == 0) {
        int64_t rh = a.tile_base[2 * t], rc = a.tile_base[2 * t + 1];
        for (int q = 0; q < kTileRows; ++q) {
            const int64_t h = hs[q], c = cs[q];
            hs[q] = rh; cs[q] = rc;
            rh += h; rc += c;
        }
    }
    __syncthreads();
    if (!heavy) return;
    const int64_t slot = hs[tid], base = cs[tid];
    if (slot >= a.cap) return;
    a.heavy[3 * slot] = rl; a.heavy[3 * slot + 1] = nch; a.heavy[3 * slot + 2] = base;
    for (int64_t c = 0; c < nch && base + c < a.cap; ++c) a.chunk_slot[base + c] = int32_t(slot);
}

// 4. light rows: one wave per row, 4 rows per wave; fp64 loss partial per block
template <int G>
__global__ __launch_bounds__(256) void sampled_rows_kernel(SArgs a)
{
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, sub = lane % G;
    const int64_t ch = kChunk << int(a.hdr[0]);
    Perm sig, tau;
    sampler_keys(a.seed, a.offset + draw_of(a), uint32_t(a.n), sig, tau);
    double lsum = 0.0;
    for (int q = 0; q < kBlockRows / 4; ++q) {
        const int rl = int(blockIdx.x) * kBlockRows + wv * (kBlockRows / 4) + q;
        if (rl >= a.n_local) break;
        int deg, tdeg;
        const int64_t L = pair_count(a, rl, deg, tdeg);
        if (L > ch) continue;                                              // heavy: chunks
        const int64_t rg = a.row_begin + rl;
        const uint32_t sig_r = perm_fwd(sig, uint32_t(rg));
        gae::v4f zr = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
        if (sub * 4 < a.DP) zr = *reinterpret_cast<const gae::v4f *>(a.Zt + rg * a.DP + sub * 4);
        process_pairs<G>(a, sig, tau, rl, 0, L, deg, tdeg, sig_r, zr, acc, lsum);
        if (a.dZ) {
            reduce_groups<G>(acc);
            if (lane < G) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = lane * 4 + u;
                    if (k < a.d) a.dZ[int64_t(rl) * a.lddz + k] = acc[u] * a.inv_n2f * mask_of(a, rg, k);
                }
            }
        }
    }
    lsum = wave_sum(lsum);
    if (lane == 0) red[wv] = lsum;
    __syncthreads();
    if (threadIdx.x == 0) a.block_loss[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// 5. chunks of heavy rows: persistent waves, chunk q -> its partial dZ row and loss
template <int G>
__global__ __launch_bounds__(256) void sampled_chunks_kernel(SArgs a)
{
    const int64_t total = a.hdr[1];
    if (total == 0) return;
    const int lane = threadIdx.x & 63, sub = lane % G;
    const int64_t ch = kChunk << int(a.hdr[0]);
    Perm sig, tau;
    sampler_keys(a.seed, a.offset + draw_of(a), uint32_t(a.n), sig, tau);
    const int64_t nw = int64_t(gridDim.x) * 4;
    for (int64_t q = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); q < total; q += nw) {
        const int64_t slot = a.chunk_slot[q];
        const int rl = int(a.heavy[3 * slot]);
        const int64_t c = q - a.heavy[3 * slot + 2];
        int deg, tdeg;
        const int64_t L = pair_count(a, rl, deg, tdeg);
        const int64_t p0 = c * ch, p1 = min(L, p0 + ch);
        const int64_t rg = a.row_begin + rl;
        const uint32_t sig_r = perm_fwd(sig, uint32_t(rg));
        gae::v4f zr = {0.f, 0.f, 0.f, 0.f}, acc = {0.f, 0.f, 0.f, 0.f};
        if (sub * 4 < a.DP) zr = *reinterpret_cast<const gae::v4f *>(a.Zt + rg * a.DP + sub * 4);
        double lsum = 0.0;
        process_pairs<G>(a, sig, tau, rl, p0, p1, deg, tdeg, sig_r, zr, acc, lsum);
        reduce_groups<G>(acc);
        if (lane < G && lane * 4 < a.DP) *reinterpret_cast<gae::v4f *>(a.cpart + q * a.DP + lane * 4) = acc;
        lsum = wave_sum(lsum);
        if (lane == 0) a.closs[q] = lsum;
    }
}

// 6. heavy rows: chunk partials added in chunk order -> dZ row, the row's loss
__global__ __launch_bounds__(256) void sampled_heavy_kernel(SArgs a)
{
    const int64_t total = a.hdr[2];
    const int lane = threadIdx.x & 63;
    const int64_t nw = int64_t(gridDim.x) * 4;
    for (int64_t slot = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6); slot < total; slot += nw) {
        const int rl = int(a.heavy[3 * slot]);
        const int64_t nch = a.heavy[3 * slot + 1], base = a.heavy[3 * slot + 2];
        const int64_t rg = a.row_begin + rl;
        if (a.dZ && lane < a.d) {
            float s = 0.f;
            for (int64_t c = 0; c < nch; ++c) s += a.cpart[(base + c) * a.DP + lane];
            a.dZ[int64_t(rl) * a.lddz + lane] = s * a.inv_n2f * mask_of(a, rg, lane);
        }
        if (lane == 0) {
            double l = 0.0;
            for (int64_t c = 0; c < nch; ++c) l += a.closs[base + c];
            a.hloss[slot] = l;
        }
    }
}

// 7. one block: block partials, then heavy rows' losses, in order; the draw counter advances
__global__ __launch_bounds__(1024) void sampled_finalize_kernel(SArgs a)
{
    __shared__ double red[16];
    const int tid = threadIdx.x;
    const int64_t nh = a.hdr[2];
    double s = 0.0;
    for (int64_t q = tid; q < a.n_b3; q += 1024) s += a.block_loss[q];
    for (int64_t q = tid; q < nh; q += 1024) s += a.hloss[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        *a.loss_out = a.hdr[3] ? __builtin_nanf("") : float(t * a.inv_n2);
        if (a.draw_dev) *a.draw_dev += 1;
    }
}

__global__ void sampled_empty_kernel(float *loss_out, uint64_t *draw_dev)
{
    *loss_out = 0.f;
    if (draw_dev) *draw_dev += 1;
}

// THE workspace layout: the launch shapes and regions of `a`, carved from `c`; the bytes walked are the size (no slack).
// hdr is a fixed 256 bytes.
int64_t sampled_layout(int64_t n, int64_t n_local, int64_t d, gae::Carver c, SArgs &a)
{
    a.DP = int((d + 3) / 4 * 4);
    a.n_tiles = int((n_local + kTileRows - 1) / kTileRows);
    a.n_b3 = int((n_local + kBlockRows - 1) / kBlockRows);
    a.cap = n_local / 16 + 1024;
    a.Zt = c.take<float>(n * a.DP);
    a.tile_cnt = c.take<int32_t>(int64_t(a.n_tiles) * 2 * kLevels);
    a.tile_base = c.take<int64_t>(int64_t(a.n_tiles) * 2);
    a.hdr = c.raw<int64_t>(256);
    a.block_loss = c.take<double>(a.n_b3);
    a.heavy = c.take<int64_t>(a.cap * 3);
    a.chunk_slot = c.take<int32_t>(a.cap);
    a.cpart = c.take<float>(a.cap * a.DP);
    a.closs = c.take<double>(a.cap);
    a.hloss = c.take<double>(a.cap);
    return c.bytes();
}

template <int G>
int launch_pairs(const SArgs &a, hipStream_t s, int grid4, int grid5)
{
    hipLaunchKernelGGL(sampled_rows_kernel<G>, dim3(unsigned(a.n_b3)), dim3(256), 0, s, a);
    GAE_CHECK_LAUNCH("sampled_rows_kernel");
    hipLaunchKernelGGL(sampled_chunks_kernel<G>, dim3(unsigned(grid4)), dim3(256), 0, s, a);
    GAE_CHECK_LAUNCH("sampled_chunks_kernel");
    hipLaunchKernelGGL(sampled_heavy_kernel, dim3(unsigned(grid5)), dim3(256), 0, s, a);
    GAE_CHECK_LAUNCH("sampled_heavy_kernel");
    return GAE_OK;
}

} // namespace

extern "C" int gae_decoder_bce_sampled(const float *Z, float *mask, int64_t ldz, int64_t n, int64_t d,
                                       int64_t row_begin, int64_t n_local, int64_t m, const int32_t *indptr,
                                       const int32_t *indices, const int32_t *t_indptr, const int32_t *t_indices,
                                       float pos_weight, float dropout_p, uint64_t seed, uint64_t offset,
                                       uint64_t *draw_dev, float *loss_out, float *dZ, int64_t lddz,
                                       int32_t *partners_out, void *workspace, int64_t *workspace_bytes, void *stream)
{
    GAE_REQUIRE(n > 0 && d > 0, GAE_E_SIZE, "gae_decoder_bce_sampled: n and d must be positive");
    GAE_REQUIRE(n < (int64_t(1) << 31), GAE_E_SIZE, "gae_decoder_bce_sampled: n = %lld beyond the int32 CSR",
                (long long)n);
    GAE_REQUIRE(d <= 64, GAE_E_RANGE, "gae_decoder_bce_sampled: d = %lld > 64", (long long)d);
    GAE_REQUIRE(row_begin >= 0 && n_local >= 0 && row_begin + n_local <= n, GAE_E_SIZE,
                "gae_decoder_bce_sampled: row window [%lld, %lld) outside [0, %lld)", (long long)row_begin,
                (long long)(row_begin + n_local), (long long)n);
    GAE_REQUIRE(m >= 1 && m <= n, GAE_E_RANGE, "gae_decoder_bce_sampled: m = %lld samples per row outside 1..%lld",
                (long long)m, (long long)n);
    GAE_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, GAE_E_RANGE,
                "gae_decoder_bce_sampled: dropout_p = %g outside [0, 1)", double(dropout_p));
    GAE_REQUIRE(ldz >= d && (!dZ || lddz >= d), GAE_E_SIZE, "gae_decoder_bce_sampled: leading dimension too small");
    GAE_REQUIRE(!dZ || n_local == 0 || t_indptr, GAE_E_NULL,
                "gae_decoder_bce_sampled: the gradient needs the CSR of A^T");
    GAE_REQUIRE(workspace_bytes, GAE_E_NULL, "gae_decoder_bce_sampled: workspace_bytes is NULL");
    SArgs a;
    const int64_t total = sampled_layout(n, n_local, d, gae::Carver(workspace), a);
    if (!workspace) {                               // size query: no device work
        *workspace_bytes = total;
        return GAE_OK;
    }
    GAE_REQUIRE(dropout_p == 0.f || mask, GAE_E_NULL, "gae_decoder_bce_sampled: dropout_p > 0 needs the mask output buffer");
    GAE_REQUIRE(Z && loss_out && (n_local == 0 || indptr), GAE_E_NULL, "gae_decoder_bce_sampled: NULL pointer");
    GAE_REQUIRE(*workspace_bytes >= total, GAE_E_WORKSPACE, "gae_decoder_bce_sampled: workspace of %lld bytes, %lld needed",
                (long long)*workspace_bytes, (long long)total);
    GAE_REQUIRE(gae::aligned16(workspace), GAE_E_ALIGN, "gae_decoder_bce_sampled: workspace not 16-byte aligned");
    hipStream_t s = gae::as_stream(stream);
    if (n_local == 0) {
        hipLaunchKernelGGL(sampled_empty_kernel, dim3(1), dim3(1), 0, s, loss_out, draw_dev);
        GAE_CHECK_LAUNCH("sampled_empty_kernel");
        return GAE_OK;
    }
    a.Z = Z; a.mask = mask; a.ldz = ldz; a.n = int(n); a.d = int(d); a.m = int(m);
    a.row_begin = row_begin; a.n_local = int(n_local);
    a.indptr = indptr; a.indices = indices; a.t_indptr = t_indptr; a.t_indices = t_indices;
    a.pw = pos_weight; a.drop_p = dropout_p; a.drop_scale = dropout_p > 0.f ? 1.0f / (1.0f - dropout_p) : 1.f;
    a.inv_n2 = 1.0 / (double(n) * double(n)); a.inv_n2f = float(a.inv_n2);
    a.seed = seed; a.offset = offset; a.draw_dev = draw_dev;
    a.loss_out = loss_out; a.dZ = dZ; a.lddz = lddz; a.partners_out = partners_out; a.grad = dZ != nullptr;
    const int64_t prep_blocks = (n * a.DP + kPrepElems - 1) / kPrepElems;
    const int64_t g1 = prep_blocks > a.n_tiles ? prep_blocks : a.n_tiles;
    GAE_REQUIRE(g1 < (int64_t(1) << 31), GAE_E_SIZE, "gae_decoder_bce_sampled: grid too large");
    hipLaunchKernelGGL(sampled_prep_count_kernel, dim3(unsigned(g1)), dim3(256), 0, s, a, int(prep_blocks));
    GAE_CHECK_LAUNCH("sampled_prep_count_kernel");
    hipLaunchKernelGGL(sampled_scan_kernel, dim3(1), dim3(1024), 0, s, a);
    GAE_CHECK_LAUNCH("sampled_scan_kernel");
    hipLaunchKernelGGL(sampled_place_kernel, dim3(unsigned(a.n_tiles)), dim3(256), 0, s, a);
    GAE_CHECK_LAUNCH("sampled_place_kernel");
    const int64_t waves_cap = (a.cap + 3) / 4;
    const int grid4 = int(waves_cap < 4096 ? waves_cap : 4096), grid5 = int(waves_cap < 1024 ? waves_cap : 1024);
    const int G = a.DP <= 4 ? 1 : a.DP <= 8 ? 2 : a.DP <= 16 ? 4 : a.DP <= 32 ? 8 : 16;
    int rc;
    switch (G) {
    case 1: rc = launch_pairs<1>(a, s, grid4, grid5); break;
    case 2: rc = launch_pairs<2>(a, s, grid4, grid5); break;
    case 4: rc = launch_pairs<4>(a, s, grid4, grid5); break;
    case 8: rc = launch_pairs<8>(a, s, grid4, grid5); break;
    default: rc = launch_pairs<16>(a, s, grid4, grid5); break;
    }
    if (rc) return rc;
    hipLaunchKernelGGL(sampled_finalize_kernel, dim3(1), dim3(1024), 0, s, a);
    GAE_CHECK_LAUNCH("sampled_finalize_kernel");
    return GAE_OK;
}
