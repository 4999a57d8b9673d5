// K23: k-means over the rows of an embedding, on the device (ops.kmeans, ops.kmeans_assign, GAE.cluster_nodes).
//
// X fp32 [n, d] (ldx), centres C fp32 [k, d] dense; 1 <= d <= 64, 1 <= k <= 256, k <= n < 2^31.
//
// One Lloyd iteration (gae_kmeans_step) is FOUR ordinary launches, none of which waits on another block:
//   assign  row i -> argmin_c |x_i - c_c|^2, evaluated as h_c - x_i . c_c with h_c = |c_c|^2 / 2.  The products run on
//           the fp32 matrix core through the tile of decoder_pairs.h: a wave's panel of 32 rows is the B operand, tiles
//           of 32 centres the A operand, read from an LDS image of C that the block stages once (rows 2 DH + 4 floats
//           apart, features past d and centres past k zeroed) next to h.  All 16 accumulators of a lane belong to ONE
//           row: the lane keeps a running (best, index) with a strict <, over its registers and tiles in ascending
//           centre order, and meets the other lane half of its row in one shuffle -- ties (equal fp32 values, duplicate
//           centres) go to the lower index, centres >= k are never candidates.  The chosen centre's distance is then
//           taken directly, sum_f (x_if - c_af)^2 as an fmaf chain in ascending f from 0.f: no cancellation of the
//           expanded form reaches dist2 or the inertia.  Labels that differ from the ones found on entry (-1 included)
//           are counted with an integer atomic in LDS; one count per block goes to the workspace.
//   sums    block b owns the rows [b R, (b + 1) R); R and the grid are functions of n alone (kNumCu is a constant, no
//           device query).  Every LDS accumulator (c, f) has exactly one writer thread -- centre c belongs to lane
//           group c mod (groups per block), feature f to a lane of the group -- which walks the block's rows in
//           ascending order.  The block's [k, d] sums, its counts and the fp64 sum of its rows' dist2 (thread t adds
//           rows t, t + 256, ... in order, then a fixed halving tree) land in the workspace.  No float atomics.
//   fold    one block per centre: the P block partials of each feature are added in the order of common.h's
//           sum_partials (its <= 32 form or its 64-lane form), the counts as int64; new centre = sum / count, written in
//           place; a centre without rows keeps its value.  Its |c_new - c_old|^2 is an fp64 chain in ascending f.
//   finish  one wave: shift2 = the centres' terms added in ascending c (fp64), inertia = the block sums in the 64-lane
//           order (fp64), changed and empty as integers; iterations += 1; done = changed == 0 || shift2 <= tol_abs.
// Every kernel of a step returns at once when status.done is set: iterations can be enqueued in groups, and the
// result has the same bits whatever the group size.  Sums, centres, inertia and shift2 are functions of (X's values,
// C, n, d, k) alone: the same bits run to run and for any ldx.
//
// Seeding (gae_kmeans_init_pp): k-means++ as an exponential race -- round r picks argmax_i mind2_i / (-log u_i), the
// lowest i among equal keys, u_i from philox4x32_10(ctr = i, draw = r, key) --: no prefix sum, no host round trip, and
// a pick that does not depend on grid or block shape.  One launch per round; its first step folds the previous
// round's per-block (key, index) candidates (every block does, redundantly).
//
// LDS: assign k_pad (2 DH + 4) 4 + k_pad 4 bytes (70.7 KB at k = 256, d > 32: two blocks of four waves per CU of the 160
// KB; 11.3 KB at d <= 16); sums k d 4 + k 4 + 2 KB (68.6 KB at most).  Accumulators in VGPRs (-amdgpu-mfma-vgpr-form,
// _build.py): the epilogue compares every one.
#include "decoder_pairs.h"

namespace {

using namespace gae::pairs;

constexpr int kNumCu = 256;            // MI355X; the constant xw.hip sizes its one-block-per-CU slots with
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / gae::kWave;
constexpr int kMaxD = 64, kMaxK = 256;
constexpr int kSumRows = 64;           // rows per block of the sums launch, at least
constexpr int kSumAhead = 16;          // ... and how many of them a thread has in flight
constexpr int kSumBlocks = 2 * kNumCu; // ... and blocks at most
constexpr int kSeedBlocks = 1024;      // blocks of a seeding round at most

struct Cand { float key; int32_t idx; };

// ---- what both sides derive from (n, d, k)
struct Plan {
    int DH, ktiles;
    int64_t panels;
    int assign_blocks;
    size_t assign_lds, sums_lds;
    int64_t R, P;                      // sums: rows per block, blocks
    int64_t seed_rows, seed_blocks;
    // the workspace regions (NULL when the plan was made for the size query) and their total
    float *dist2, *psum;               // dist2 of a step; mind2 of the seeding
    int32_t *changed_part, *pcount, *empty_c;
    double *pinertia, *shift_c;
    Cand *cand;                        // the seeding's two candidate lists
    int64_t need;
};

using gae::cdiv;
using gae::launch_lds;
using gae::up256;

// the checks, the launch shapes and THE workspace layout, carved from `ws` (NULL: counted only)
int plan(const char *fn, int64_t n, int64_t d, int64_t k, void *ws, Plan &p)
{
    GAE_REQUIRE(d >= 1 && d <= kMaxD, GAE_E_RANGE, "%s: d = %lld outside 1..64", fn, (long long)d);
    GAE_REQUIRE(k >= 1 && k <= kMaxK, GAE_E_RANGE, "%s: k = %lld outside 1..256", fn, (long long)k);
    GAE_REQUIRE(n >= 0, GAE_E_SIZE, "%s: negative n = %lld", fn, (long long)n);
    GAE_REQUIRE(n < (int64_t(1) << 31), GAE_E_SIZE, "%s: n = %lld beyond int32 labels", fn, (long long)n);
    GAE_REQUIRE(k <= n, GAE_E_SIZE, "%s: k = %lld centres for n = %lld rows", fn, (long long)k, (long long)n);
    p.DH = dh_of(d);
    p.ktiles = int(cdiv(k, kTile));
    p.panels = cdiv(n, kRows);
    const int64_t ab = cdiv(p.panels, kWaves);
    p.assign_blocks = int(ab < 2 * kNumCu ? ab : 2 * kNumCu);
    const int64_t kpad = int64_t(p.ktiles) * kTile;
    p.assign_lds = size_t(kpad * (2 * p.DH + 4) * 4 + kpad * 4 + 16);
    p.sums_lds = size_t(k * d * 4 + k * 4 + 8 + kThreads * 8);
    const int64_t r = cdiv(n, kSumBlocks);
    p.R = r > kSumRows ? r : kSumRows;
    p.P = cdiv(n, p.R);
    const int64_t sb = cdiv(n, kThreads);
    p.seed_rows = cdiv(n, sb < kSeedBlocks ? sb : kSeedBlocks);
    p.seed_blocks = cdiv(n, p.seed_rows);
    // sized by bounds of P and the seeding grid that never shrink as n grows: the query is monotone in n
    const int64_t pmax = cdiv(n, kSumRows) < kSumBlocks ? cdiv(n, kSumRows) : kSumBlocks;
    const int64_t smax = sb < kSeedBlocks ? sb : kSeedBlocks;
    gae::Carver c(ws);
    p.dist2 = c.take<float>(n);
    p.changed_part = c.take<int32_t>(2 * kNumCu);
    p.psum = c.take<float>(pmax * k * d);
    p.pcount = c.take<int32_t>(pmax * k);
    p.pinertia = c.take<double>(pmax);
    p.shift_c = c.take<double>(k);
    p.empty_c = c.take<int32_t>(k);
    p.cand = c.take<Cand>(2 * smax);
    p.need = c.bytes();
    return GAE_OK;
}

// ---------------------------------------------------------------------------------------------------- assign
struct AssignArgs {
    const float *X;
    int64_t ldx;
    int n, d, k, ktiles;
    int64_t panels;
    const float *C;
    int32_t *labels;
    float *dist2;                      // NULL: not wanted
    int32_t *changed_part;             // NULL: predict -- `labels` is output only
    const gae_kmeans_status *status;   // NULL: predict
};

template <int DH>
__global__ __launch_bounds__(kThreads) void kmeans_assign_kernel(const AssignArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (a.status && a.status->done) return;
    constexpr int pitch = 2 * DH + 4;
    const int kpad = a.ktiles * kTile;
    float *cs = lds;                                   // [kpad][pitch]: the A operand's image of C
    float *hs = cs + kpad * pitch;                     // [kpad]: |c|^2 / 2
    int *chg = reinterpret_cast<int *>(hs + kpad);
    for (int e = threadIdx.x; e < kpad * 2 * DH; e += kThreads) {
        const int c = e / (2 * DH), f = e % (2 * DH);
        cs[c * pitch + f] = c < a.k && f < a.d ? a.C[int64_t(c) * a.d + f] : 0.f;
    }
    if (threadIdx.x == 0) *chg = 0;
    __syncthreads();
    for (int c = threadIdx.x; c < kpad; c += kThreads) {
        float s = 0.f;
        for (int f = 0; f < a.d; ++f) s = fmaf(cs[c * pitch + f], cs[c * pitch + f], s);
        hs[c] = 0.5f * s;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, col = lane & 31, h = lane >> 5;
    int changed = 0;
    for (int64_t panel = int64_t(blockIdx.x) * kWaves + wave; panel < a.panels; panel += int64_t(gridDim.x) * kWaves) {
        const int64_t row = panel * kRows + col;
        const bool row_in = row < a.n;
        const float *xp = a.X + (row_in ? row : int64_t(a.n) - 1) * a.ldx;       // a row past n is clamped, never stored
        float zb[DH];
#pragma unroll
        for (int s = 0; s < DH; ++s) {
            const int f = feat0<DH>(0, h) + s;
            const float v = xp[f < a.d ? f : a.d - 1];
            zb[s] = f < a.d ? v : 0.f;
        }
        float best = INFINITY;
        int bi = 0;
        for (int t = 0; t < a.ktiles; ++t) {
            float za[DH];
            const float *cp = cs + (t * kTile + col) * pitch + feat0<DH>(0, h);
#pragma unroll
            for (int s = 0; s < DH; ++s) za[s] = cp[s];
            const v16f acc = mma<DH>(zero_acc(), za, zb);
#pragma unroll
            for (int r = 0; r < 16; ++r) {             // ascending centres: the strict < keeps the lowest of equals
                const int c = tile_col(t * kTile, r, h);
                const float v = hs[c] - acc[r];
                if (c < a.k && v < best) { best = v; bi = c; }
            }
        }
        const float ob = __shfl_xor(best, 32, 64);     // the other lane half of this row
        const int oi = __shfl_xor(bi, 32, 64);
        if (ob < best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        if (h == 0 && row_in) {
            const float *cc = cs + bi * pitch;
            float dist = 0.f;
            for (int f = 0; f < a.d; ++f) {
                const float df = xp[f] - cc[f];
                dist = fmaf(df, df, dist);
            }
            if (a.changed_part && a.labels[row] != bi) ++changed;
            a.labels[row] = bi;
            if (a.dist2) a.dist2[row] = dist;
        }
    }
    if (a.changed_part) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) changed += __shfl_down(changed, off, 64);
        if (lane == 0 && changed) atomicAdd(chg, changed);
        __syncthreads();
        if (threadIdx.x == 0) a.changed_part[blockIdx.x] = *chg;
    }
}

int launch_assign(const Plan &p, const AssignArgs &a, hipStream_t st)
{
    return dispatch(a.d, [&](auto dh, auto) {          // d <= 64: always one chunk
        return launch_lds<&kmeans_assign_kernel<dh>>("kmeans_assign_kernel", p.assign_blocks, kThreads, p.assign_lds, st,
                                                     a);
    });
}

// ---------------------------------------------------------------------------------------------------- sums
struct SumsArgs {
    const float *X;
    int64_t ldx;
    int n, d, k, dp;                   // dp: the power of two >= d, lanes per group
    int64_t R;
    const int32_t *labels;
    const float *dist2;
    float *psum;                       // [P][k d]
    int32_t *pcount;                   // [P][k]
    double *pinertia;                  // [P]
    const gae_kmeans_status *status;
};

__global__ __launch_bounds__(kThreads) void kmeans_sums_kernel(const SumsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    if (a.status->done) return;
    const int kd = a.k * a.d;
    float *acc = lds;                                                  // [k][d]
    int *cnt = reinterpret_cast<int *>(acc + kd);                      // [k]
    double *red = reinterpret_cast<double *>(lds + (kd + a.k + 1) / 2 * 2);    // [kThreads]
    for (int e = threadIdx.x; e < kd + a.k; e += kThreads) lds[e] = 0.f;       // (+0.f and int 0 share their bits)
    __syncthreads();

    const int64_t r0 = int64_t(blockIdx.x) * a.R;
    const int64_t r1 = r0 + a.R < a.n ? r0 + a.R : int64_t(a.n);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int groups = kThreads / a.dp;                                // lane groups per block, a power of two
    const int gid = wave * (64 / a.dp) + lane / a.dp, f = lane % a.dp;
    const bool f_in = f < a.d;
    // centre c is summed by group c mod groups, feature f by the group's lane f: one writer per accumulator, rows ascending
    for (int64_t i0 = r0; i0 < r1; i0 += kSumAhead) {
        // labels and X values of kSumAhead rows in flight at once; the X load does not wait for the label (every group
        // loads the row, the owner adds it)
        int lab[kSumAhead];
        float v[kSumAhead];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) {
            const int64_t i = i0 + u < r1 ? i0 + u : r1 - 1;
            lab[u] = i0 + u < r1 ? a.labels[i] : -1;
            v[u] = f_in ? a.X[i * a.ldx + f] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) {
            if (f_in && unsigned(lab[u]) < unsigned(a.k) && (lab[u] & (groups - 1)) == gid) {
                acc[lab[u] * a.d + f] += v[u];
                if (f == 0) cnt[lab[u]] += 1;
            }
        }
    }
    double s = 0.0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += kThreads) s += double(a.dist2[i]);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int e = threadIdx.x; e < kd; e += kThreads) a.psum[int64_t(blockIdx.x) * kd + e] = acc[e];
    for (int c = threadIdx.x; c < a.k; c += kThreads) a.pcount[int64_t(blockIdx.x) * a.k + c] = cnt[c];
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (int(threadIdx.x) < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.pinertia[blockIdx.x] = red[0];
}

// ---------------------------------------------------------------------------------------------------- fold, finish
struct FoldArgs {
    float *C;
    int d, k;
    int64_t P;
    const float *psum;
    const int32_t *pcount;
    double *shift_c;                   // [k]
    int32_t *empty_c;                  // [k]
    const gae_kmeans_status *status;
};

__global__ __launch_bounds__(kThreads) void kmeans_fold_kernel(const FoldArgs a)
{
    __shared__ float ssum[kMaxD];
    __shared__ double sd[kMaxD];
    __shared__ unsigned long long scount;
    if (a.status->done) return;
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t stride = int64_t(a.k) * a.d;
    if (threadIdx.x == 0) scount = 0;
    __syncthreads();
    const int L = gae::partial_lanes(a.P);
    if (L == 64) {
        for (int f = wave; f < a.d; f += kWaves) {                     // all 64 lanes of the wave call
            const float s = gae::sum_partials(a.psum + int64_t(c) * a.d + f, a.P, stride, lane, 64);
            if (lane == 0) ssum[f] = s;
        }
    } else if (int(threadIdx.x) < a.d) {
        ssum[threadIdx.x] = gae::sum_partials(a.psum + int64_t(c) * a.d + threadIdx.x, a.P, stride, 0, 1);
    }
    unsigned long long mine = 0;
    for (int64_t q = threadIdx.x; q < a.P; q += kThreads) mine += unsigned(a.pcount[q * a.k + c]);
    if (mine) atomicAdd(&scount, mine);                                // integers: any order
    __syncthreads();
    const unsigned long long count = scount;
    if (int(threadIdx.x) < a.d) {
        double term = 0.0;
        if (count > 0) {
            float *cp = a.C + int64_t(c) * a.d + threadIdx.x;
            const float nw = ssum[threadIdx.x] / float(count);
            const double df = double(nw) - double(*cp);
            term = df * df;
            *cp = nw;
        }
        sd[threadIdx.x] = term;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sh = 0.0;
        for (int f = 0; f < a.d; ++f) sh += sd[f];
        a.shift_c[c] = sh;
        a.empty_c[c] = count == 0 ? 1 : 0;
    }
}

struct FinishArgs {
    gae_kmeans_status *status;
    int k, n_changed;
    int64_t P;
    const double *pinertia, *shift_c;
    const int32_t *empty_c, *changed_part;
    double tol_abs;
};

__global__ __launch_bounds__(64) void kmeans_finish_kernel(const FinishArgs a)
{
    __shared__ double ssh[kMaxK];
    if (a.status->done) return;
    const int lane = threadIdx.x;
    double inertia = 0.0;
    for (int64_t q = lane; q < a.P; q += 64) inertia += a.pinertia[q];
    long long changed = 0, empty = 0;
    for (int b = lane; b < a.n_changed; b += 64) changed += a.changed_part[b];
    for (int c = lane; c < a.k; c += 64) { empty += a.empty_c[c]; ssh[c] = a.shift_c[c]; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        inertia += __shfl_down(inertia, off, 64);
        changed += __shfl_down(changed, off, 64);
        empty += __shfl_down(empty, off, 64);
    }
    __syncthreads();
    if (lane == 0) {
        double shift2 = 0.0;
        for (int c = 0; c < a.k; ++c) shift2 += ssh[c];
        gae_kmeans_status *st = a.status;
        st->iterations += 1;
        st->changed = changed;
        st->empty = empty;
        st->inertia = inertia;
        st->shift2 = shift2;
        st->done = changed == 0 || shift2 <= a.tol_abs ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------- seeding
struct SeedArgs {
    const float *X;
    int64_t ldx;
    int n, d, k, round;                // round r in 1 .. k; launch k only records the pick of round k - 1
    uint64_t key;
    int64_t rows, n_prev;              // rows per block; candidates of the previous round
    float *mind2;
    const Cand *prev;
    Cand *out;
    float *C_out;
    int32_t *chosen;
};

// the larger key, the lower index among equal keys: a total order, so any fold order gives the same winner
__device__ __forceinline__ bool beats(float ka, int ia, float kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// -log u of the 24-bit draw m, u = (m + 0.5) 2^-24: both branches take an argument that fp32 holds exactly
__device__ __forceinline__ float neg_log_u(uint32_t m)
{
    if (m < (1u << 23)) return -logf((float(m) + 0.5f) * (1.0f / 16777216.0f));
    return -log1pf(-((float((1u << 24) - 1u - m) + 0.5f) * (1.0f / 16777216.0f)));
}

__global__ __launch_bounds__(kThreads) void kmeans_seed_kernel(const SeedArgs a)
{
    __shared__ float xprev[kMaxD];
    __shared__ float rk[kThreads];
    __shared__ int ri[kThreads];
    const int tid = threadIdx.x;
    // ---- the previous round's pick
    float bk = -1.f;
    int bidx = INT32_MAX;
    if (a.round == 1) {
        if (tid == 0) {
            uint32_t c[4];
            gae::philox4x32_10(0, 0, a.key, c);
            bk = 0.f; bidx = int(c[0] % uint32_t(a.n));
        }
    } else {
        for (int64_t q = tid; q < a.n_prev; q += kThreads) {
            const Cand v = a.prev[q];
            if (beats(v.key, v.idx, bk, bidx)) { bk = v.key; bidx = v.idx; }
        }
    }
    auto block_best = [&]() {
        rk[tid] = bk; ri[tid] = bidx;
        __syncthreads();
        for (int off = kThreads / 2; off > 0; off >>= 1) {
            if (tid < off && beats(rk[tid + off], ri[tid + off], rk[tid], ri[tid])) { rk[tid] = rk[tid + off]; ri[tid] = ri[tid + off]; }
            __syncthreads();
        }
    };
    block_best();
    int prev = ri[0];
    if (unsigned(prev) >= unsigned(a.n)) prev = 0;             // no key compared (NaN rows): stay inside X
    __syncthreads();
    if (tid < a.d) {
        const float v = a.X[int64_t(prev) * a.ldx + tid];
        xprev[tid] = v;
        if (blockIdx.x == 0) a.C_out[int64_t(a.round - 1) * a.d + tid] = v;
    }
    if (blockIdx.x == 0 && tid == 0) a.chosen[a.round - 1] = prev;
    __syncthreads();
    if (a.round == a.k) return;

    // ---- this round: lower mind2, draw, and the block's candidate
    bk = -1.f; bidx = INT32_MAX;
    const int64_t r0 = int64_t(blockIdx.x) * a.rows;
    const int64_t r1 = r0 + a.rows < a.n ? r0 + a.rows : int64_t(a.n);
    for (int64_t i = r0 + tid; i < r1; i += kThreads) {
        const float *xp = a.X + i * a.ldx;
        float dist = 0.f;
        for (int f = 0; f < a.d; ++f) {
            const float df = xp[f] - xprev[f];
            dist = fmaf(df, df, dist);
        }
        const float m = a.round == 1 ? dist : fminf(a.mind2[i], dist);
        a.mind2[i] = m;
        uint32_t c[4];
        gae::philox4x32_10(uint64_t(i), uint64_t(a.round), a.key, c);
        const float key = m / neg_log_u(c[0] >> 8);
        if (beats(key, int(i), bk, bidx)) { bk = key; bidx = int(i); }
    }
    block_best();
    if (tid == 0) a.out[blockIdx.x] = Cand{rk[0], ri[0]};
}

int check_x(const char *fn, const float *X, int64_t ldx, int64_t d, const void *workspace, int64_t bytes, const Plan &p)
{
    GAE_REQUIRE(ldx >= d, GAE_E_SIZE, "%s: leading dimension too small (ldx %lld < d)", fn, (long long)ldx);
    GAE_REQUIRE(X, GAE_E_NULL, "%s: X is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    GAE_REQUIRE(bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn, (long long)bytes,
                (long long)p.need);
    return GAE_OK;
}

} // namespace

extern "C" int64_t gae_kmeans_workspace_bytes(int64_t n, int64_t d, int64_t k)
{
    Plan p;
    if (const int rc = plan("gae_kmeans_workspace_bytes", n, d, k, nullptr, p)) return rc;
    return p.need;
}

extern "C" int gae_kmeans_assign(const float *X, int64_t ldx, int64_t n, int64_t d, const float *C, int64_t k,
                                 int32_t *labels_out, float *dist2_out, void *workspace, int64_t workspace_bytes,
                                 void *stream)
{
    const char *fn = "gae_kmeans_assign";
    Plan p;
    if (const int rc = plan(fn, n, d, k, workspace, p)) return rc;
    if (const int rc = check_x(fn, X, ldx, d, workspace, workspace_bytes, p)) return rc;
    GAE_REQUIRE(C && labels_out, GAE_E_NULL, "%s: C / labels_out is NULL", fn);
    const AssignArgs a{X, ldx, int(n), int(d), int(k), p.ktiles, p.panels, C, labels_out, dist2_out, nullptr, nullptr};
    return launch_assign(p, a, gae::as_stream(stream));
}

extern "C" int gae_kmeans_step(const float *X, int64_t ldx, int64_t n, int64_t d, float *C, int64_t k, int32_t *labels,
                               gae_kmeans_status *status, double tol_abs, int flags, void *workspace,
                               int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_kmeans_step";
    Plan p;
    if (const int rc = plan(fn, n, d, k, workspace, p)) return rc;
    GAE_REQUIRE(flags == 0, GAE_E_RANGE, "%s: unknown flags 0x%x", fn, flags);
    GAE_REQUIRE(tol_abs == tol_abs, GAE_E_RANGE, "%s: tol_abs is NaN", fn);
    if (const int rc = check_x(fn, X, ldx, d, workspace, workspace_bytes, p)) return rc;
    GAE_REQUIRE(C && labels && status, GAE_E_NULL, "%s: C / labels / status is NULL", fn);
    hipStream_t st = gae::as_stream(stream);

    const AssignArgs aa{X, ldx, int(n), int(d), int(k), p.ktiles, p.panels, C, labels, p.dist2, p.changed_part, status};
    if (const int rc = launch_assign(p, aa, st)) return rc;
    int dp = 1;
    while (dp < d) dp *= 2;
    const SumsArgs sa{X, ldx, int(n), int(d), int(k), dp, p.R, labels, p.dist2, p.psum, p.pcount, p.pinertia, status};
    if (const int rc = launch_lds<&kmeans_sums_kernel>("kmeans_sums_kernel", p.P, kThreads, p.sums_lds, st, sa)) return rc;
    const FoldArgs fa{C, int(d), int(k), p.P, p.psum, p.pcount, p.shift_c, p.empty_c, status};
    hipLaunchKernelGGL(kmeans_fold_kernel, dim3(unsigned(k)), dim3(kThreads), 0, st, fa);
    GAE_CHECK_LAUNCH("kmeans_fold_kernel");
    const FinishArgs na{status, int(k), p.assign_blocks, p.P, p.pinertia, p.shift_c, p.empty_c, p.changed_part, tol_abs};
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3(1), dim3(64), 0, st, na);
    GAE_CHECK_LAUNCH("kmeans_finish_kernel");
    return GAE_OK;
}

extern "C" int gae_kmeans_init_pp(const float *X, int64_t ldx, int64_t n, int64_t d, int64_t k, uint64_t seed,
                                  float *C_out, int32_t *chosen_out, void *workspace, int64_t workspace_bytes,
                                  void *stream)
{
    const char *fn = "gae_kmeans_init_pp";
    Plan p;
    if (const int rc = plan(fn, n, d, k, workspace, p)) return rc;
    if (const int rc = check_x(fn, X, ldx, d, workspace, workspace_bytes, p)) return rc;
    GAE_REQUIRE(C_out && chosen_out, GAE_E_NULL, "%s: C_out / chosen_out is NULL", fn);
    SeedArgs a{X, ldx, int(n), int(d), int(k), 0, seed ^ 0x9E3779B97F4A7C15ull, p.seed_rows, p.seed_blocks,
               p.dist2, nullptr, nullptr, C_out, chosen_out};
    hipStream_t st = gae::as_stream(stream);
    for (int r = 1; r <= int(k); ++r) {
        a.round = r;
        a.prev = p.cand + ((r - 1) & 1) * p.seed_blocks;       // two lists: a round reads one while it writes the other
        a.out = p.cand + (r & 1) * p.seed_blocks;
        hipLaunchKernelGGL(kmeans_seed_kernel, dim3(unsigned(r == int(k) ? 1 : p.seed_blocks)), dim3(kThreads), 0, st, a);
        GAE_CHECK_LAUNCH("kmeans_seed_kernel");
    }
    return GAE_OK;
}
