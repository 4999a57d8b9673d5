// K15: per-member decoder + weighted BCE of a batched graph (GAE.reconstruction_loss(g, scope="graph")).
//
// The reference's Trainer.iteration (gae_dgl/train_inductive.py:44-48) scores one molecule g alone as
//   l_g = (1 / n_g^2) sum_{i,j in g} [(1 - y_ij) x_ij + (1 + (pw_g - 1) y_ij) softplus(-x_ij)],
//   x_ij = zt_i . zt_j (Zt = Z (.) mask, gae.py:70), y_ij = #edges j -> i inside g, pw_g = (n_g^2 - S_g) / S_g,
// and this launch returns loss = (1 / G') sum_g l_g over the G' members with S_g > 0, its gradient and every l_g.
// The pairs BETWEEN two members -- all but ~2e-6 of the N^2 pairs of a 4096-molecule batch -- are never formed.
//
// Math.  term(x, y) = softplus(x) + y [(pw - 1) softplus(-x) - x].  Over a whole member sum_ij y_ij f(x_ij) =
// sum_ij y_ji f(x_ij) (x is symmetric), so every pair is weighted by w_ij / 2, w_ij = y_ij + y_ji: ONE label count per
// pair serves the loss and the gradient
//   dZt_i = (1 / (G' n_g^2)) sum_j c_ij zt_j,  c_ij = C_ij + C_ji = 2 sigmoid(x_ij) - w_ij (1 + (pw - 1) sigmoid(-x_ij)).
// A panel's rows see y_ij through the CSR (rows = destination) and y_ji through the CSR of A^T: the panel owns the
// whole gradient of its rows, no cross-block gradient reduction.
//
// Layout.  One 256-thread workgroup per (member, 64-row panel); a ZINC molecule (<= 38 atoms) is one panel.  The panel
// keeps its rows of Zt in LDS and streams the member's columns in 64-row tiles: the labels of the tile are counted
// into an LDS tile (integer atomics: exact), the 64 x 64 logits are exact fp32 FMA chains (k-ordered, VALU), the
// coefficients replace the counts in place and c Zt is accumulated per row in registers.  No cross-member pair, no
// bf16 split, no range guard: ~2e6 logits per 4096-molecule batch.
//
// Grid.  Work items are handed out by a ticket (atomic counter), so a block waits only for work items that started
// before it: items [0, n_chunks) count S_g of 64 members each (the structural prologue that G' needs), then one item
// per member (its panel 0), then -- only when the host bound max_graph_nodes exceeds 64 -- one item per 64-row chunk
// of the batch: chunk j owns the extra panel (k >= 1) of the member that starts in rows [64 j, 64 j + 64), of which
// there is at most one (two extra panels in one chunk would be < 64 rows apart).  The grid is O(total panels), not
// O(G x max n_g): one 20 000-node member among 4 000 molecules adds ~1 800 items, not 4 000 x 313.
//
// Reduction.  Every panel item stores its fp64 loss partial; the last block to finish (done counter) folds each
// member's panels in panel order, divides by n_g^2 and averages over G' in fp64.  No float atomics: bit-identical
// run to run.  The same block advances the dropout draw counter and puts the counters back to zero.
//
// Hand-offs between workgroups follow the write-through form: the payload (S_g, partials) is stored sc1 (agent-scope
// relaxed atomic stores), every storing wave drains (vmcnt 0) before its workgroup's barrier, one lane signals by an
// agent-scope atomic add, the consumer polls relaxed and reads the payload with sc1 loads only.  Every spin is bounded:
// a give-up sets the timeout word and the loss comes back NaN.
#include "common.h"

namespace {

constexpr int kT = 64;              // panel rows = column-tile width
constexpr int kThreads = 256;
constexpr int kChunk = 64;          // members per structural work item
constexpr unsigned kSpinLimit = 1u << 22;   // x s_sleep 8 (~0.2 us): gives up after ~1 s

typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) unsigned long long gu64;
#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// the caller's zero-initialised counters (gae_decoder_bce_graphs: sync_dev); every launch leaves them zero
enum { kTicket = 0, kDone = 1, kChunksDone = 2, kValid = 3, kTimeout = 4, kSyncWords = 8 };

struct GraphsArgs {
    const float *Z;
    float *mask;
    int64_t ldz, n;
    int d;
    int n_chunks;
    const int64_t *node_ptr;
    int64_t G, extra;               // members; extra panel items (0 unless max_graph_nodes > 64)
    const int32_t *indptr, *indices, *t_indptr, *t_indices;
    const int64_t *counts;
    float p, scale;
    uint64_t seed, offset;
    uint64_t *draw_dev;
    float *loss_out, *graph_loss_out, *dZ;
    int64_t lddz;
    double *partial;                // [G + extra]
    int64_t *S;                     // [G]
    unsigned *sync;
};

__device__ __forceinline__ unsigned ld_u32(const unsigned *p) { return __hip_atomic_load((gu32 *)p, RLX_AGENT); }
__device__ __forceinline__ uint64_t ld_u64(const void *p) { return __hip_atomic_load((gu64 *)p, RLX_AGENT); }
__device__ __forceinline__ void st_u64(void *p, uint64_t v) { __hip_atomic_store((gu64 *)p, (unsigned long long)v, RLX_AGENT); }
__device__ __forceinline__ unsigned add_u32(unsigned *p, unsigned v) { return __hip_atomic_fetch_add((gu32 *)p, v, RLX_AGENT); }
__device__ __forceinline__ void drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// the inverted-dropout multiplier of element (i, k): gae_dropout_mask's stream (element e = i d + k, quad e / 4) when
// the mask is drawn here, else the given mask (or 1)
__device__ __forceinline__ float multiplier(const GraphsArgs &a, int64_t i, int k, uint64_t draw)
{
    if (a.p > 0.f) {
        const int64_t e = i * a.d + k;
        uint32_t c[4];
        gae::philox4x32_10(a.offset + uint64_t(e >> 2), draw, a.seed, c);
        const uint32_t bits = (e & 2) ? ((e & 1) ? c[3] : c[2]) : ((e & 1) ? c[1] : c[0]);
        return gae::dropout_multiplier(bits, a.p, a.scale);
    }
    return a.mask ? a.mask[i * a.ldz + k] : 1.f;
}

// true rows of the batch: counts[0] for a fixed-capacity batch
__device__ __forceinline__ int64_t valid_rows(const GraphsArgs &a)
{
    if (!a.counts) return a.n;
    const int64_t v = a.counts[0];
    return v < 0 ? 0 : (v > a.n ? a.n : v);
}

// a member takes part when its range is sane and lies inside the true rows
__device__ __forceinline__ bool covered(int64_t p0, int64_t p1, int64_t n_valid)
{
    return p0 >= 0 && p0 <= p1 && p1 <= n_valid;
}

// fixed-order block sum (all threads call; result valid in every thread)
__device__ __forceinline__ double block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// thread 0 waits (bounded) until the structural items have published; returns G'
__device__ unsigned wait_chunks(const GraphsArgs &a)
{
    unsigned spins = 0;
    while (ld_u32(&a.sync[kChunksDone]) < unsigned(a.n_chunks)) {
        if (++spins > kSpinLimit) {
            add_u32(&a.sync[kTimeout], 1u);
            break;
        }
        __builtin_amdgcn_s_sleep(8);
    }
    return ld_u32(&a.sync[kValid]);
}

// ---- structural item: S_g of members [c * 64, c * 64 + 64) and how many of them count
__device__ void chunk_item(const GraphsArgs &a, int c, int64_t n_valid)
{
    __shared__ int64_t lo[kChunk], hi[kChunk], e0[kChunk], scan[kChunk + 1];
    __shared__ int cnt[kChunk];
    const int tid = threadIdx.x;
    const int64_t g0 = int64_t(c) * kChunk;
    const int gc = int(a.G - g0 < kChunk ? a.G - g0 : kChunk);
    if (tid < gc) {
        const int64_t p0 = a.node_ptr[g0 + tid], p1 = a.node_ptr[g0 + tid + 1];
        const bool cov = covered(p0, p1, n_valid);
        lo[tid] = p0; hi[tid] = p1;
        e0[tid] = cov ? a.indptr[p0] : 0;
        scan[tid + 1] = cov ? int64_t(a.indptr[p1]) - a.indptr[p0] : 0;     // edge count, scanned below
        cnt[tid] = 0;
    }
    __syncthreads();
    if (tid == 0) {
        scan[0] = 0;
        for (int l = 0; l < gc; ++l) scan[l + 1] += scan[l];
    }
    __syncthreads();
    const int64_t total = scan[gc];
    for (int64_t v0 = tid; v0 < total; v0 += int64_t(kThreads) * 4) {
        int32_t col[4];
        int mem[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {           // four independent loads in flight
            const int64_t v = v0 + int64_t(u) * kThreads;
            mem[u] = -1;
            if (v < total) {
                int l = 0, r = gc;               // last l with scan[l] <= v
                while (r - l > 1) { const int m = (l + r) >> 1; if (scan[m] <= v) l = m; else r = m; }
                mem[u] = l;
                col[u] = a.indices[e0[l] + (v - scan[l])];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (mem[u] >= 0 && col[u] >= lo[mem[u]] && col[u] < hi[mem[u]]) atomicAdd(&cnt[mem[u]], 1);
    }
    __syncthreads();
    __shared__ int n_ok;
    if (tid == 0) n_ok = 0;
    __syncthreads();
    if (tid < gc) {
        const int64_t s = cnt[tid];
        st_u64(&a.S[g0 + tid], uint64_t(s));
        if (covered(lo[tid], hi[tid], n_valid) && hi[tid] > lo[tid] && s > 0) atomicAdd(&n_ok, 1);
    }
    drain();
    __syncthreads();
    if (tid == 0) {
        add_u32(&a.sync[kValid], unsigned(n_ok));
        add_u32(&a.sync[kChunksDone], 1u);
    }
}

// ---- panel item: the rows [p0 + 64 k, ...) of member g for k in [k_begin, k_end)
template <int DP>
__device__ double panel_item(const GraphsArgs &a, int64_t g, int64_t k_begin, int64_t k_end, int64_t n_valid,
                             uint64_t draw, double *red)
{
    constexpr int LD = DP + 1;                   // odd row pitch: conflict-free column walks
    constexpr int NA = DP / 4;                   // features per thread in the c Zt product
    __shared__ float Zp[kT * LD], Zc_buf[kT * LD];
    __shared__ union { int w; float c; } W[kT * (kT + 1)];
    __shared__ int64_t ro[kT + 1], tro[kT + 1];
    __shared__ int64_t s_S;
    __shared__ int s_cnt;
    __shared__ unsigned s_gv;
    const int tid = threadIdx.x;
    const int64_t p0 = a.node_ptr[g], p1 = a.node_ptr[g + 1];
    const bool cov = covered(p0, p1, n_valid);
    const int64_t n_g = cov ? p1 - p0 : 0;
    const int64_t n_panels = (n_g + kT - 1) / kT;
    if (!cov) {
        // left out (a member that ends behind the true rows of a fixed-capacity batch): zero gradient, rows clipped
        if (a.dZ) {
            int64_t b = p0 + k_begin * kT, e = k_end == INT64_MAX ? p1 : p0 + k_end * kT;
            e = e < p1 ? e : p1;
            b = b < 0 ? 0 : b;
            e = e < a.n ? e : a.n;
            for (int64_t q = tid; q < (e - b) * a.d; q += kThreads)
                a.dZ[(b + q / a.d) * a.lddz + q % a.d] = 0.f;
        }
        return 0.0;
    }
    if (k_end > n_panels) k_end = n_panels;
    if (k_begin >= k_end) return 0.0;
    // pos_weight needs S_g of the whole member: a one-panel member counts it below, a larger one takes the prologue's
    bool waited = false;
    unsigned gv = 0;
    if (tid == 0) s_S = -1;
    if (n_panels > 1) {
        if (tid == 0) { s_gv = wait_chunks(a); s_S = int64_t(ld_u64(&a.S[g])); }
        waited = true;
    }
    __syncthreads();
    if (waited) gv = s_gv;
    double loss_acc = 0.0;
    for (int64_t k = k_begin; k < k_end; ++k) {
        const int64_t r0 = p0 + k * kT;
        const int nr = int(p1 - r0 < kT ? p1 - r0 : kT);
        // rows of the panel: Zt and the CSR / CSR^T row offsets
        for (int q = tid; q < kT * DP; q += kThreads) {
            const int r = q / DP, kk = q % DP;
            float v = 0.f;
            if (r < nr && kk < a.d) v = a.Z[(r0 + r) * a.ldz + kk] * multiplier(a, r0 + r, kk, draw);
            Zp[r * LD + kk] = v;
        }
        if (tid <= nr) ro[tid] = int64_t(a.indptr[r0 + tid]) - a.indptr[r0];
        else if (tid >= 128 && tid - 128 <= nr) tro[tid - 128] = int64_t(a.t_indptr[r0 + tid - 128]) - a.t_indptr[r0];
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        const int64_t eb = a.indptr[r0], teb = a.t_indptr[r0];
        const int64_t ne = ro[nr], nte = tro[nr];
        float acc[NA];
#pragma unroll
        for (int m = 0; m < NA; ++m) acc[m] = 0.f;
        const int rr = tid >> 2, kq = tid & 3;       // c Zt product: row rr, features kq + 4 m
        const int ta = tid >> 4, tb = tid & 15;      // logits: rows ta + 16 i, columns tb + 16 j
        for (int64_t c0 = p0; c0 < p1; c0 += kT) {
            const int nc = int(p1 - c0 < kT ? p1 - c0 : kT);
            const float *Zc = Zp;
            if (c0 != r0) {
                for (int q = tid; q < kT * DP; q += kThreads) {
                    const int r = q / DP, kk = q % DP;
                    float v = 0.f;
                    if (r < nc && kk < a.d) v = a.Z[(c0 + r) * a.ldz + kk] * multiplier(a, c0 + r, kk, draw);
                    Zc_buf[r * LD + kk] = v;
                }
                Zc = Zc_buf;
            }
            for (int q = tid; q < kT * (kT + 1); q += kThreads) W[q].w = 0;
            __syncthreads();
            // labels of the tile: w_rc = y_ij + y_ji (in-edges of the panel rows, then their out-edges)
            const bool first = c0 == p0;
            int own = 0;
            for (int64_t v = tid; v < ne + nte; v += kThreads) {
                const bool t = v >= ne;
                const int64_t vv = t ? v - ne : v;
                const int64_t *off = t ? tro : ro;
                int l = 0, h = nr;                   // last row with off[l] <= vv
                while (h - l > 1) { const int m = (l + h) >> 1; if (off[m] <= vv) l = m; else h = m; }
                const int64_t col = t ? a.t_indices[teb + vv] : a.indices[eb + vv];
                if (first && !t && col >= p0 && col < p1) ++own;        // S_g of a one-panel member
                const int64_t cc = col - c0;
                if (cc >= 0 && cc < nc) atomicAdd(&W[l * (kT + 1) + int(cc)].w, 1);
            }
            if (first && n_panels == 1 && own) atomicAdd(&s_cnt, own);
            __syncthreads();
            if (first && n_panels == 1 && tid == 0) s_S = s_cnt;
            __syncthreads();
            const int64_t S = s_S;
            if (S <= 0) break;                       // no edge inside the member: left out (zero gradient)
            const double pw = (double(n_g) * double(n_g) - double(S)) / double(S);   // train_inductive.py:46
            const float pwm1 = float(pw) - 1.f;
            // logits, loss terms, coefficients (in place of the counts)
            float tile_loss = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = ta + 16 * i;
                if (r >= nr) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = tb + 16 * j;
                    if (c >= nc) continue;
                    float x = 0.f;
#pragma unroll
                    for (int kk = 0; kk < DP; ++kk) x = __builtin_fmaf(Zp[r * LD + kk], Zc[c * LD + kk], x);
                    const float w = float(W[r * (kT + 1) + c].w);
                    const float e = __expf(-fabsf(x));
                    const float inv = 1.f / (1.f + e);
                    const float sig_p = x >= 0.f ? inv : e * inv;      // sigmoid(x)
                    const float sig_m = x >= 0.f ? e * inv : inv;      // sigmoid(-x)
                    const float l1p = log1pf(e);
                    const float sp_p = fmaxf(x, 0.f) + l1p;            // softplus(x)
                    const float sp_m = fmaxf(-x, 0.f) + l1p;           // softplus(-x)
                    tile_loss += sp_p + 0.5f * w * (pwm1 * sp_m - x);
                    W[r * (kT + 1) + c].c = 2.f * sig_p - w * (1.f + pwm1 * sig_m);
                }
            }
            loss_acc += double(tile_loss);
            __syncthreads();
            if (rr < nr) {
                for (int c = 0; c < nc; ++c) {
                    const float cf = W[rr * (kT + 1) + c].c;
#pragma unroll
                    for (int m = 0; m < NA; ++m) acc[m] = __builtin_fmaf(cf, Zc[c * LD + kq + 4 * m], acc[m]);
                }
            }
            __syncthreads();
        }
        // the panel's rows of dZ = dZt (.) mask, scaled by 1 / (G' n_g^2) once G' is known
        if (a.dZ) {
            const bool left_out = s_S <= 0;
            if (!waited && !left_out) {
                if (tid == 0) s_gv = wait_chunks(a);
                __syncthreads();
                gv = s_gv;
                waited = true;
            }
            const float scale = left_out || gv == 0 ? 0.f : float(1.0 / (double(gv) * double(n_g) * double(n_g)));
            if (rr < nr) {
#pragma unroll
                for (int m = 0; m < NA; ++m) {
                    const int kk = kq + 4 * m;
                    if (kk < a.d) {
                        const float v = left_out ? 0.f : acc[m] * scale * multiplier(a, r0 + rr, kk, draw);
                        a.dZ[(r0 + rr) * a.lddz + kk] = v;
                    }
                }
            }
        }
        if (s_S <= 0) loss_acc = 0.0;
        __syncthreads();
    }
    return block_sum(loss_acc, red);
}

// ---- the last block: per-member losses, the mean over G', counters back to zero, the draw counter advanced
__device__ void fold(const GraphsArgs &a, int64_t n_valid, double *red)
{
    const int tid = threadIdx.x;
    const unsigned gv = ld_u32(&a.sync[kValid]);
    const unsigned timeout = ld_u32(&a.sync[kTimeout]);
    double sum = 0.0;
    for (int64_t g = tid; g < a.G; g += kThreads) {
        const int64_t p0 = a.node_ptr[g], p1 = a.node_ptr[g + 1];
        const int64_t S = int64_t(ld_u64(&a.S[g]));
        const bool ok = covered(p0, p1, n_valid) && p1 > p0 && S > 0;
        float out = __builtin_nanf("");
        if (ok) {
            const uint64_t b0 = ld_u64(&a.partial[g]);
            double s = __builtin_bit_cast(double, b0);
            if (a.extra > 0) {
                const int64_t np = (p1 - p0 + kT - 1) / kT;
                for (int64_t k = 1; k < np; ++k)
                    s += __builtin_bit_cast(double, ld_u64(&a.partial[a.G + (p0 + k * kT) / kT]));
            }
            const double lg = s / (double(p1 - p0) * double(p1 - p0));
            sum += lg;
            out = float(lg);
        }
        if (a.graph_loss_out) a.graph_loss_out[g] = out;
    }
    const double total = block_sum(sum, red);
    if (tid == 0) {
        a.loss_out[0] = (gv > 0 && !timeout) ? float(total / double(gv)) : __builtin_nanf("");
        if (a.p > 0.f && a.draw_dev) *a.draw_dev += 1;
        for (int q = 0; q < kSyncWords; ++q) __hip_atomic_store((gu32 *)&a.sync[q], 0u, RLX_AGENT);
    }
}

template <int DP>
__global__ __launch_bounds__(kThreads) void bce_graphs_kernel(const GraphsArgs a)
{
    __shared__ double red[kThreads];
    __shared__ unsigned s_ticket;
    __shared__ int64_t s_item[2];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    if (tid == 0) s_ticket = add_u32(&a.sync[kTicket], 1u);
    const uint64_t draw = (a.p > 0.f && a.draw_dev) ? *a.draw_dev : 0;
    const int64_t n_valid = valid_rows(a);
    // ---- duties of every block, independent of its work item: the mask of this draw over all n x d elements
    //      (gae_dropout_mask's layout), and zero gradient for the rows outside [p_0, p_G)
    const int64_t stride = int64_t(gridDim.x) * kThreads, first = int64_t(blockIdx.x) * kThreads + tid;
    if (a.p > 0.f) {
        const int64_t ne = a.n * a.d, nq = (ne + 3) / 4;
        for (int64_t q = first; q < nq; q += stride) {
            uint32_t c[4];
            gae::philox4x32_10(a.offset + uint64_t(q), draw, a.seed, c);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t e = q * 4 + u;
                if (e < ne) a.mask[(e / a.d) * a.ldz + e % a.d] = gae::dropout_multiplier(c[u], a.p, a.scale);
            }
        }
    }
    if (a.dZ) {
        int64_t lo = a.G > 0 ? a.node_ptr[0] : a.n, hi = a.G > 0 ? a.node_ptr[a.G] : a.n;
        lo = lo < 0 ? 0 : (lo > a.n ? a.n : lo);
        hi = hi < lo ? lo : (hi > a.n ? a.n : hi);
        const int64_t n_out = (lo + (a.n - hi)) * a.d;
        for (int64_t q = first; q < n_out; q += stride) {
            const int64_t r = q / a.d, row = r < lo ? r : hi + (r - lo);
            a.dZ[row * a.lddz + q % a.d] = 0.f;
        }
    }
    __syncthreads();
    const int64_t t = s_ticket;
    if (t < a.n_chunks) {
        chunk_item(a, int(t), n_valid);
    } else if (t - a.n_chunks < a.G + a.extra) {
        const int64_t w = t - a.n_chunks;
        // the work item -> (member, first panel, end panel)
        if (tid == 0) {
            int64_t g = -1, kb = 0, ke = 0;
            if (w < a.G) {
                g = w; kb = 0; ke = a.extra > 0 ? 1 : INT64_MAX;    // no extra items: panel 0's block walks them all
            } else {
                const int64_t s0 = (w - a.G) * kT;
                int64_t l = 0, h = a.G;                // last member with node_ptr[l] <= s0
                if (a.node_ptr[0] <= s0) {
                    while (h - l > 1) { const int64_t m = (l + h) >> 1; if (a.node_ptr[m] <= s0) l = m; else h = m; }
                    const int64_t p0 = a.node_ptr[l], p1 = a.node_ptr[l + 1];
                    const int64_t k = (s0 - p0 + kT - 1) / kT;
                    if (k >= 1 && p0 + k * kT < p1) { g = l; kb = k; ke = k + 1; }
                }
            }
            s_item[0] = g; s_item[1] = kb;
            s_last = int(ke == INT64_MAX ? -1 : ke);
        }
        __syncthreads();
        const int64_t g = s_item[0], kb = s_item[1];
        const int64_t ke = s_last < 0 ? INT64_MAX : s_last;
        const double part = g >= 0 ? panel_item<DP>(a, g, kb, ke, n_valid, draw, red) : 0.0;
        if (tid == 0) st_u64(&a.partial[w], __builtin_bit_cast(uint64_t, part));
    }
    // ---- done: the last block to get here folds (every block's stores drained before its add)
    drain();
    __syncthreads();
    if (tid == 0) s_last = add_u32(&a.sync[kDone], 1u) == gridDim.x - 1u;
    __syncthreads();
    if (s_last) fold(a, n_valid, red);
}

inline int64_t extra_items(int64_t n, int64_t max_graph_nodes) { return max_graph_nodes > kT ? (n + kT - 1) / kT : 0; }

} // namespace

extern "C" int64_t gae_decoder_bce_graphs_workspace_bytes(int64_t n, int64_t n_graphs, int64_t max_graph_nodes, int64_t d)
{
    if (n < 0 || n_graphs < 0 || max_graph_nodes < 0 || d < 0) return GAE_E_SIZE;
    if (d > 64) return GAE_E_RANGE;
    const int64_t items = n_graphs + extra_items(n, max_graph_nodes);
    return (items + n_graphs) * 8 + 64;
}

extern "C" int gae_decoder_bce_graphs(const float *Z, float *mask, int64_t ldz, int64_t n, int64_t d,
                                      const int64_t *node_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                                      const int32_t *indptr, const int32_t *indices, const int32_t *t_indptr,
                                      const int32_t *t_indices, const int64_t *counts_dev, float dropout_p,
                                      uint64_t seed, uint64_t offset, uint64_t *draw_dev, float *loss_out,
                                      float *graph_loss_out, float *dZ, int64_t lddz, void *workspace,
                                      int64_t workspace_bytes, uint32_t *sync_dev, void *stream)
{
    GAE_REQUIRE(n >= 0 && d >= 0 && n_graphs >= 0 && max_graph_nodes >= 0, GAE_E_SIZE,
                "gae_decoder_bce_graphs: negative size");
    GAE_REQUIRE(d <= 64, GAE_E_RANGE, "gae_decoder_bce_graphs: d = %lld (at most 64)", (long long)d);
    GAE_REQUIRE(n < (int64_t(1) << 31) && n_graphs < (int64_t(1) << 30), GAE_E_SIZE,
                "gae_decoder_bce_graphs: n = %lld / %lld graphs beyond the int32 CSR", (long long)n, (long long)n_graphs);
    GAE_REQUIRE(ldz >= d && (!dZ || lddz >= d), GAE_E_SIZE, "gae_decoder_bce_graphs: leading dimension too small");
    GAE_REQUIRE(node_ptr || n_graphs == 0, GAE_E_NULL, "gae_decoder_bce_graphs: node_ptr is NULL");
    GAE_REQUIRE(loss_out && sync_dev, GAE_E_NULL, "gae_decoder_bce_graphs: loss_out / sync_dev is NULL");
    GAE_REQUIRE(n == 0 || (indptr && t_indptr), GAE_E_NULL, "gae_decoder_bce_graphs: CSR / CSR of A^T is NULL");
    GAE_REQUIRE(n == 0 || d == 0 || Z, GAE_E_NULL, "gae_decoder_bce_graphs: Z is NULL");
    GAE_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, GAE_E_RANGE, "gae_decoder_bce_graphs: dropout_p = %g outside [0, 1)",
                double(dropout_p));
    GAE_REQUIRE(dropout_p == 0.f || mask || n * d == 0, GAE_E_NULL,
                "gae_decoder_bce_graphs: in-launch dropout needs the [n, d] mask output");
    const int64_t need = gae_decoder_bce_graphs_workspace_bytes(n, n_graphs, max_graph_nodes, d);
    GAE_REQUIRE(workspace_bytes >= need && (workspace || need == 0), GAE_E_WORKSPACE,
                "gae_decoder_bce_graphs: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)need);
    GraphsArgs a;
    a.Z = Z; a.mask = mask; a.ldz = ldz; a.n = n; a.d = int(d);
    a.node_ptr = node_ptr; a.G = n_graphs; a.extra = extra_items(n, max_graph_nodes);
    a.n_chunks = int((n_graphs + kChunk - 1) / kChunk);
    a.indptr = indptr; a.indices = indices; a.t_indptr = t_indptr; a.t_indices = t_indices;
    a.counts = counts_dev;
    a.p = dropout_p; a.scale = 1.0f / (1.0f - dropout_p); a.seed = seed; a.offset = offset; a.draw_dev = draw_dev;
    a.loss_out = loss_out; a.graph_loss_out = graph_loss_out; a.dZ = dZ; a.lddz = lddz;
    a.partial = reinterpret_cast<double *>(workspace);
    a.S = reinterpret_cast<int64_t *>(a.partial + (n_graphs + a.extra));
    a.sync = sync_dev;
    const int64_t items = int64_t(a.n_chunks) + n_graphs + a.extra;
    const unsigned grid = unsigned(items > 0 ? items : 1);
    hipStream_t s = gae::as_stream(stream);
    if (d <= 16)
        hipLaunchKernelGGL(bce_graphs_kernel<16>, dim3(grid), dim3(kThreads), 0, s, a);
    else if (d <= 32)
        hipLaunchKernelGGL(bce_graphs_kernel<32>, dim3(grid), dim3(kThreads), 0, s, a);
    else
        hipLaunchKernelGGL(bce_graphs_kernel<64>, dim3(grid), dim3(kThreads), 0, s, a);
    GAE_CHECK_LAUNCH("bce_graphs_kernel");
    return GAE_OK;
}
