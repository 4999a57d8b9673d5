// K35 / K36: neighbourhood link-prediction baselines (ops.neighbour_scores, ops.neighbour_topk): common neighbours,
// Jaccard, Adamic-Adar and resource allocation over a symmetric CSR, without the n x n two-hop matrix.
//
// THE CONTRACT (the K35 / K36 comment of include/gae_hip_experimental.h has it in full).
//   GRAPH    int32 indptr [n + 1], indices [nnz]; rows ascending, duplicates kept; symmetric (the wrapper checks).
//   Gamma(i) the DISTINCT columns of row i other than i: duplicate edges and self-loops do not count.  deg(i) = |Gamma(i)|.
//   PAIR     common(i, j) = |Gamma(i) & Gamma(j)|;  wsum_c(i, j) = sum of W[w, c] over w in Gamma(i) & Gamma(j), for nw <= 2
//            caller-supplied int64 weight columns (fixed point, 32 fraction bits: the kernels add integers, nothing else).
//   TOP-K    candidates of query row i: every j != i with common(i, j) >= 1, minus Gamma(i) under EXCLUDE_EDGES.  Key: common
//            (cn), wsum (aa, ra), the bits of the fp64 quotient double(common) / double(deg_i + deg_j - common) (jaccard; a
//            non-negative double orders as its bits).  Order: better() of topk_heap.h -- larger key first, then lower j.
//            Fewer than k candidates: index -1, common 0, wsum 0 at the tail.
//
// Launches (ordinary ones; integer LDS and global atomics only, no float is accumulated anywhere):
//   degrees  one thread per row: deg, and the status bits of a column outside [0, n) / a row that is not ascending.
//   pairs    eight lanes per pair: the shorter row is spread over the lanes, each lane skips duplicates, the self columns and
//            binary-searches the longer row; the integers meet in three xor shuffles.  A hub row loops.
//   plan     one thread per query row: B_i = sum of rowlen(w) over w in Gamma(i); rows with 2 B_i <= table_slots go to the short
//            list, the others to the long list (the workspace); a row with B_i = 0 is padded here.
//   short    one wave per listed row: an LDS hash table keyed by j (linear probing, at most table_slots probes, an error bit
//            instead of a spin), the count by a 32-bit and the sum by a 64-bit LDS integer add.
//   long     four waves per listed row: the candidate columns in windows of table_slots, dense LDS accumulators indexed by
//            j - window base; every Gamma(w) is entered by binary search at the window start, and the next window starts at the
//            smallest column any of them has left (never before the end of this one), so empty stretches cost nothing.
//   Both then drop j in Gamma(i) when excluding edges, form the key and select by RANK: the order is total and strict, so
//   the number of candidates better than (key, j) is its output position.  No heap, no order of arrival: both routes, every
//   table_slots and every schedule give the same bits.  The long route keeps the k best so far beside each window.
//
// SAFETY: a row pointer outside [0, nnz] reads as an empty row; a column outside [0, n) is never used as an index; a window
// entry is checked against the window; every probe and window loop is bounded.
#include "common.h"
#include "topk_heap.h"

namespace {

using gae::cdiv;
using gae::topk::better;

constexpr int kGroup = 8;                  // lanes per pair (K35) and per neighbour row of the short route
constexpr int kMaxK = GAE_NEIGHBOUR_MAX_K;
constexpr int kMaxSlots = 2048;
constexpr int kLongThreads = 256;

struct Csr {
    const int32_t *indptr, *indices;
    int n;
    int64_t nnz;
};

__device__ __forceinline__ void row_span(const Csr &g, int r, int &b, int &e)
{
    int64_t s = g.indptr[r], t = g.indptr[r + 1];
    if (s < 0 || t < s || t > g.nnz) s = t = 0;
    b = int(s); e = int(t);
}

// the entry at position p of row r (which starts at b) is a member of Gamma(r): in range, not r, not a repeat
__device__ __forceinline__ bool member(const Csr &g, int r, int b, int p, int c)
{
    return unsigned(c) < unsigned(g.n) && c != r && (p == b || g.indices[p - 1] != c);
}

// first position in [b, e) whose column is >= v
__device__ __forceinline__ int lower_bound(const int32_t *idx, int b, int e, int v)
{
    while (b < e) {
        const int m = b + ((e - b) >> 1);
        if (idx[m] < v) b = m + 1; else e = m;
    }
    return b;
}

// ---------------------------------------------------------------------------------------------------- degrees
__global__ __launch_bounds__(256) void neighbour_degrees_kernel(const Csr g, int32_t *deg, int64_t *status)
{
    const int64_t r64 = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (r64 >= g.n) return;
    const int r = int(r64);
    const int64_t s = g.indptr[r], t = g.indptr[r + 1];
    int64_t bits = 0;
    if (s < 0 || t < s || t > g.nnz) bits |= GAE_NEIGHBOUR_ERR_INDPTR;
    int b, e;
    row_span(g, r, b, e);
    int d = 0;
    for (int p = b; p < e; ++p) {
        const int c = g.indices[p];
        if (unsigned(c) >= unsigned(g.n)) bits |= GAE_NEIGHBOUR_ERR_COLUMN;
        if (p > b && g.indices[p - 1] > c) bits |= GAE_NEIGHBOUR_ERR_ORDER;
        d += member(g, r, b, p, c) ? 1 : 0;
    }
    deg[r] = d;
    if (bits) gae::or_bits(status, bits);
}

// ---------------------------------------------------------------------------------------------------- pairs
struct PairArgs {
    Csr g;
    const int32_t *pi, *pj;
    int64_t m;
    const int64_t *W;
    int nw;
    int32_t *common;
    int64_t *wsum;
    int64_t *status;
};

__global__ __launch_bounds__(256) void neighbour_pairs_kernel(const PairArgs a)
{
    const int64_t q = (int64_t(blockIdx.x) * 256 + threadIdx.x) / kGroup;
    const int l = threadIdx.x & (kGroup - 1);
    const bool live = q < a.m;
    const int i = live ? a.pi[q] : 0, j = live ? a.pj[q] : 0;
    const bool ok = live && unsigned(i) < unsigned(a.g.n) && unsigned(j) < unsigned(a.g.n);
    int common = 0;
    int64_t s0 = 0, s1 = 0;
    if (ok) {
        int ib, ie, jb, je;
        row_span(a.g, i, ib, ie);
        row_span(a.g, j, jb, je);
        const bool i_short = ie - ib <= je - jb;
        const int rs = i_short ? i : j, ro = i_short ? j : i;              // the spread row, the searched row
        const int sb = i_short ? ib : jb, se = i_short ? ie : je, ob = i_short ? jb : ib, oe = i_short ? je : ie;
        for (int p = sb + l; p < se; p += kGroup) {
            const int c = a.g.indices[p];
            if (!member(a.g, rs, sb, p, c) || c == ro) continue;
            const int pos = lower_bound(a.g.indices, ob, oe, c);
            if (pos < oe && a.g.indices[pos] == c) {
                ++common;
                if (a.nw > 0) s0 += a.W[int64_t(c) * a.nw];
                if (a.nw > 1) s1 += a.W[int64_t(c) * a.nw + 1];
            }
        }
    }
#pragma unroll
    for (int off = kGroup / 2; off > 0; off >>= 1) {
        common += __shfl_xor(common, off, 64);
        s0 += __shfl_xor(s0, off, 64);
        s1 += __shfl_xor(s1, off, 64);
    }
    if (live && l == 0) {
        a.common[q] = ok ? common : -1;
        if (a.nw > 0) a.wsum[q * a.nw] = s0;
        if (a.nw > 1) a.wsum[q * a.nw + 1] = s1;
        if (!ok) gae::or_bits(a.status, GAE_NEIGHBOUR_ERR_QUERY);
    }
}

// ---------------------------------------------------------------------------------------------------- top-k
struct TopkArgs {
    Csr g;
    const int32_t *rows;                   // [m] or null: row q is node q
    int64_t m;
    int k, kind, exclude;
    const int64_t *w;                      // weight of node v at w[v * ldw], or null
    int64_t ldw;
    const int32_t *deg;
    int slots, log_slots;
    int32_t *index_out, *common_out;       // [m, k]
    int64_t *wsum_out;
    int64_t *status;
    int32_t *counts;                       // [2]: rows of the short and of the long list
    int32_t *short_list, *long_list;       // [m] query positions
};

// the one carve of the workspace, for the size query and the call
struct TopkPlan {
    int32_t *counts, *short_list, *long_list;
    int64_t need;
};

TopkPlan carve_topk(int64_t m, void *ws)
{
    gae::Carver c(ws);
    TopkPlan p;
    p.counts = c.take<int32_t>(2);
    p.short_list = c.take<int32_t>(m);
    p.long_list = c.take<int32_t>(m);
    p.need = c.bytes();
    return p;
}

__device__ __forceinline__ void pad_row(const TopkArgs &a, int64_t q, int from)
{
    for (int t = from; t < a.k; ++t) {
        a.index_out[q * a.k + t] = -1;
        a.common_out[q * a.k + t] = 0;
        a.wsum_out[q * a.k + t] = 0;
    }
}

__global__ __launch_bounds__(256) void neighbour_plan_kernel(const TopkArgs a)
{
    const int64_t q = int64_t(blockIdx.x) * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int route = -1;                        // 0 short, 1 long, -1 neither (no lane leaves before the ballots)
    if (q < a.m) {
        const int i = a.rows ? a.rows[q] : int(q);
        int64_t B = 0;
        if (unsigned(i) >= unsigned(a.g.n)) {
            gae::or_bits(a.status, GAE_NEIGHBOUR_ERR_QUERY);
        } else {
            int b, e;
            row_span(a.g, i, b, e);
            for (int p = b; p < e; ++p) {
                const int w = a.g.indices[p];
                if (!member(a.g, i, b, p, w)) continue;
                int wb, we;
                row_span(a.g, w, wb, we);
                B += we - wb;
            }
        }
        if (B == 0) pad_row(a, q, 0);
        else route = 2 * B <= a.slots ? 0 : 1;
    }
    // one atomic per wave and list: the lanes of a list take consecutive places behind the leader's
    for (int r = 0; r < 2; ++r) {
        const unsigned long long mask = __ballot(route == r);
        if (mask == 0) continue;
        const int leader = __ffsll(mask) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(a.counts + r, __popcll(mask));
        base = __shfl(base, leader, 64);
        if (route == r) (r == 0 ? a.short_list : a.long_list)[base + __popcll(mask & ((1ull << lane) - 1))] = int32_t(q);
    }
}

// LDS of one block: the accumulators (tkey only on the short route), the candidate list, the k best so far (long route)
struct Lds {
    int64_t *tsum, *ckey, *cws, *bkey, *bws;           // [S], [CC], [CC], [2][kMaxK], [2][kMaxK]
    int32_t *tkey, *tcnt, *cj, *ccm, *bj, *bcm, *misc; // [S], [S], [CC], [CC], [2][kMaxK], [2][kMaxK], [4]
};

constexpr int cand_capacity(int slots, bool is_long) { return is_long ? slots + kMaxK : slots / 2; }
constexpr int64_t lds_bytes(int slots, bool is_long)
{
    return int64_t(slots) * 16 + int64_t(cand_capacity(slots, is_long)) * 24 + (is_long ? 2 * kMaxK * 24 : 0) + 16;
}

__device__ __forceinline__ Lds carve_lds(void *base, int S, bool is_long)
{
    const int CC = cand_capacity(S, is_long), BB = is_long ? 2 * kMaxK : 0;
    Lds l;
    l.tsum = static_cast<int64_t *>(base);
    l.ckey = l.tsum + S;
    l.cws = l.ckey + CC;
    l.bkey = l.cws + CC;
    l.bws = l.bkey + BB;
    l.tkey = reinterpret_cast<int32_t *>(l.bws + BB);
    l.tcnt = l.tkey + S;
    l.cj = l.tcnt + S;
    l.ccm = l.cj + CC;
    l.bj = l.ccm + CC;
    l.bcm = l.bj + BB;
    l.misc = l.bcm + BB;
    return l;
}

__device__ __forceinline__ void lds_add64(int64_t *p, int64_t v)
{
    atomicAdd(reinterpret_cast<unsigned long long *>(p), static_cast<unsigned long long>(v));
}

// the key of candidate j of row i under the total order
__device__ __forceinline__ int64_t key_of(const TopkArgs &a, int deg_i, int j, int common, int64_t wsum)
{
    if (a.kind == GAE_NEIGHBOUR_CN) return common;
    if (a.kind == GAE_NEIGHBOUR_JACCARD)
        return __double_as_longlong(double(common) / double(int64_t(deg_i) + a.deg[j] - common));
    return wsum;
}

// j is an entry of row i (b .. e): under EXCLUDE_EDGES it is no candidate
__device__ __forceinline__ bool is_edge(const TopkArgs &a, int b, int e, int j)
{
    const int pos = lower_bound(a.g.indices, b, e, j);
    return pos < e && a.g.indices[pos] == j;
}

// candidate c of C gets the number of candidates better than it; emit(rank, c) for the ranks below k
template <class Emit>
__device__ __forceinline__ void rank_select(const Lds &l, int C, int k, int tid, int nt, Emit &&emit)
{
    for (int c = tid; c < C; c += nt) {
        const int64_t key = l.ckey[c];
        const int j = l.cj[c];
        int rank = 0;
        for (int d = 0; d < C; ++d) rank += better(l.ckey[d], l.cj[d], key, j) ? 1 : 0;
        if (rank < k) emit(rank, c);
    }
}

__global__ __launch_bounds__(64) void neighbour_topk_short_kernel(const TopkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int tid = threadIdx.x, S = a.slots, CC = cand_capacity(S, false);
    if (blockIdx.x == 0 && tid == 0) { a.status[1] = a.counts[0]; a.status[2] = a.counts[1]; }
    if (int(blockIdx.x) >= a.counts[0]) return;
    const Lds l = carve_lds(lds_raw, S, false);
    const int64_t q = a.short_list[blockIdx.x];
    const int i = a.rows ? a.rows[q] : int(q);
    int b, e;
    row_span(a.g, i, b, e);
    for (int s = tid; s < S; s += 64) { l.tkey[s] = -1; l.tcnt[s] = 0; l.tsum[s] = 0; }
    if (tid == 0) l.misc[0] = 0;
    __syncthreads();

    // ---- accumulate: group `sub` takes the entries sub, sub + 8, ... of row i, its eight lanes stride Gamma(w)
    const int sub = tid / kGroup, sl = tid % kGroup;
    bool full = false;
    for (int p = b + sub; p < e; p += 64 / kGroup) {
        const int w = a.g.indices[p];
        if (!member(a.g, i, b, p, w)) continue;
        const int64_t wt = a.w ? a.w[int64_t(w) * a.ldw] : 0;
        int wb, we;
        row_span(a.g, w, wb, we);
        for (int t = wb + sl; t < we; t += kGroup) {
            const int j = a.g.indices[t];
            if (!member(a.g, w, wb, t, j) || j == i) continue;
            unsigned h = (unsigned(j) * 2654435761u) >> (32 - a.log_slots);
            bool placed = false;
            for (int probe = 0; probe < S && !placed; ++probe) {
                const int old = atomicCAS(l.tkey + h, -1, j);
                if (old == -1 || old == j) {
                    atomicAdd(l.tcnt + h, 1);
                    lds_add64(l.tsum + h, wt);
                    placed = true;
                } else {
                    h = (h + 1) & unsigned(S - 1);
                }
            }
            full |= !placed;
        }
    }
    __syncthreads();

    // ---- candidates
    const int deg_i = a.deg[i];
    for (int s = tid; s < S; s += 64) {
        const int j = l.tkey[s];
        if (j < 0 || (a.exclude && is_edge(a, b, e, j))) continue;
        const int c = atomicAdd(l.misc, 1);
        if (c >= CC) { full = true; continue; }
        const int cm = l.tcnt[s];
        const int64_t ws = l.tsum[s];
        l.ckey[c] = key_of(a, deg_i, j, cm, ws);
        l.cj[c] = j; l.ccm[c] = cm; l.cws[c] = ws;
    }
    if (full) gae::or_bits(a.status, GAE_NEIGHBOUR_ERR_TABLE);
    __syncthreads();
    const int C = l.misc[0] < CC ? l.misc[0] : CC;
    rank_select(l, C, a.k, tid, 64, [&](int rank, int c) {
        a.index_out[q * a.k + rank] = l.cj[c];
        a.common_out[q * a.k + rank] = l.ccm[c];
        a.wsum_out[q * a.k + rank] = l.cws[c];
    });
    for (int t = C + tid; t < a.k; t += 64) {
        a.index_out[q * a.k + t] = -1;
        a.common_out[q * a.k + t] = 0;
        a.wsum_out[q * a.k + t] = 0;
    }
}

__global__ __launch_bounds__(kLongThreads) void neighbour_topk_long_kernel(const TopkArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int NT = kLongThreads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, S = a.slots, k = a.k;
    if (int(blockIdx.x) >= a.counts[1]) return;
    const Lds l = carve_lds(lds_raw, S, true);
    const int64_t q = a.long_list[blockIdx.x];
    const int i = a.rows ? a.rows[q] : int(q);
    int b, e;
    row_span(a.g, i, b, e);
    const int deg_i = a.deg[i];
    int T = 0, cur = 0;                    // the k best so far: T entries of buffer cur, best first
    int base = 0;
    // windows [base, base + S): base grows by at least S per turn, so at most n / S + 1 turns
    while (base < a.g.n) {
        for (int s = tid; s < S; s += NT) { l.tcnt[s] = 0; l.tsum[s] = 0; }
        if (tid == 0) { l.misc[0] = 0; l.misc[1] = INT32_MAX; }
        __syncthreads();
        // ---- accumulate: wave v takes the entries v, v + 4, ... of row i, its lanes stride Gamma(w) inside the window
        for (int p = b + wave; p < e; p += NT / 64) {
            const int w = a.g.indices[p];
            if (!member(a.g, i, b, p, w)) continue;
            const int64_t wt = a.w ? a.w[int64_t(w) * a.ldw] : 0;
            int wb, we;
            row_span(a.g, w, wb, we);
            const int lo = lower_bound(a.g.indices, wb, we, base), hi = lower_bound(a.g.indices, lo, we, base + S);
            for (int t = lo + lane; t < hi; t += 64) {
                const int j = a.g.indices[t];
                if (!member(a.g, w, wb, t, j) || j == i || j < base || j >= base + S) continue;
                atomicAdd(l.tcnt + (j - base), 1);
                lds_add64(l.tsum + (j - base), wt);
            }
            if (lane == 0 && hi < we) atomicMin(l.misc + 1, a.g.indices[hi]);
        }
        __syncthreads();
        // ---- candidates of the window that can still enter the k best, then the k best so far
        const int64_t worst_key = T == k ? l.bkey[cur * kMaxK + k - 1] : 0;
        const int worst_j = T == k ? l.bj[cur * kMaxK + k - 1] : 0;
        for (int s = tid; s < S; s += NT) {
            const int cm = l.tcnt[s];
            if (cm == 0) continue;
            const int j = base + s;
            if (j >= a.g.n || (a.exclude && is_edge(a, b, e, j))) continue;
            const int64_t ws = l.tsum[s];
            const int64_t key = key_of(a, deg_i, j, cm, ws);
            if (T == k && !better(key, j, worst_key, worst_j)) continue;
            const int c = atomicAdd(l.misc, 1);
            l.ckey[c] = key; l.cj[c] = j; l.ccm[c] = cm; l.cws[c] = ws;
        }
        __syncthreads();
        const int W = l.misc[0];
        const int next = l.misc[1];
        if (W > 0) {
            for (int t = tid; t < T; t += NT) {
                l.ckey[W + t] = l.bkey[cur * kMaxK + t]; l.cj[W + t] = l.bj[cur * kMaxK + t];
                l.ccm[W + t] = l.bcm[cur * kMaxK + t]; l.cws[W + t] = l.bws[cur * kMaxK + t];
            }
            __syncthreads();
            const int C = W + T, o = (cur ^ 1) * kMaxK;
            rank_select(l, C, k, tid, NT, [&](int rank, int c) {
                l.bkey[o + rank] = l.ckey[c]; l.bj[o + rank] = l.cj[c];
                l.bcm[o + rank] = l.ccm[c]; l.bws[o + rank] = l.cws[c];
            });
            T = C < k ? C : k;
            cur ^= 1;
        }
        __syncthreads();
        if (next == INT32_MAX) break;
        base = next > base + S ? next : base + S;
    }
    for (int t = tid; t < k; t += NT) {
        const bool have = t < T;
        a.index_out[q * k + t] = have ? l.bj[cur * kMaxK + t] : -1;
        a.common_out[q * k + t] = have ? l.bcm[cur * kMaxK + t] : 0;
        a.wsum_out[q * k + t] = have ? l.bws[cur * kMaxK + t] : 0;
    }
}

// ---------------------------------------------------------------------------------------------------- host checks
int check_graph(const char *fn, const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz)
{
    GAE_REQUIRE(n >= 0 && nnz >= 0, GAE_E_SIZE, "%s: negative n = %lld or nnz = %lld", fn, (long long)n, (long long)nnz);
    GAE_REQUIRE(n < (int64_t(1) << 30), GAE_E_SIZE, "%s: n = %lld is 2^30 or more (the fixed-point sums need common < 2^30)",
                fn, (long long)n);
    GAE_REQUIRE(nnz < (int64_t(1) << 31), GAE_E_SIZE, "%s: nnz = %lld beyond the int32 CSR", fn, (long long)nnz);
    GAE_REQUIRE(indptr, GAE_E_NULL, "%s: indptr is NULL", fn);
    GAE_REQUIRE(nnz == 0 || indices, GAE_E_NULL, "%s: indices is NULL", fn);
    return GAE_OK;
}

bool slots_taken(int64_t s) { return s >= 64 && s <= kMaxSlots && (s & (s - 1)) == 0; }

int check_topk_shape(const char *fn, int64_t n, int64_t m)
{
    GAE_REQUIRE(n >= 0 && m >= 0, GAE_E_SIZE, "%s: negative n = %lld or m = %lld", fn, (long long)n, (long long)m);
    GAE_REQUIRE(n < (int64_t(1) << 30) && m < (int64_t(1) << 30), GAE_E_SIZE, "%s: n = %lld or m = %lld is 2^30 or more", fn,
                (long long)n, (long long)m);
    return GAE_OK;
}

} // namespace

extern "C" int gae_neighbour_degrees(const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, int32_t *deg,
                                     int64_t *status, void *stream)
{
    const char *fn = "gae_neighbour_degrees";
    if (const int rc = check_graph(fn, indptr, indices, n, nnz)) return rc;
    GAE_REQUIRE(status, GAE_E_NULL, "%s: status is NULL", fn);
    GAE_REQUIRE(n == 0 || deg, GAE_E_NULL, "%s: deg is NULL", fn);
    if (n == 0) return GAE_OK;
    const Csr g{indptr, indices, int(n), nnz};
    hipLaunchKernelGGL(neighbour_degrees_kernel, dim3(unsigned(cdiv(n, 256))), dim3(256), 0, gae::as_stream(stream), g, deg,
                       status);
    GAE_CHECK_LAUNCH("neighbour_degrees_kernel");
    return GAE_OK;
}

extern "C" int gae_neighbour_pairs(const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, const int32_t *pair_i,
                                   const int32_t *pair_j, int64_t m, const int64_t *W, int64_t nw, int32_t *common_out,
                                   int64_t *wsum_out, int64_t *status, void *stream)
{
    const char *fn = "gae_neighbour_pairs";
    if (const int rc = check_graph(fn, indptr, indices, n, nnz)) return rc;
    GAE_REQUIRE(m >= 0 && m < (int64_t(1) << 31), GAE_E_SIZE, "%s: m = %lld outside 0 .. 2^31 - 1", fn, (long long)m);
    GAE_REQUIRE(nw >= 0 && nw <= GAE_NEIGHBOUR_MAX_WEIGHTS, GAE_E_RANGE, "%s: nw = %lld weight columns outside 0..%d", fn,
                (long long)nw, GAE_NEIGHBOUR_MAX_WEIGHTS);
    GAE_REQUIRE(status, GAE_E_NULL, "%s: status is NULL", fn);
    GAE_REQUIRE(m == 0 || (pair_i && pair_j && common_out), GAE_E_NULL, "%s: pair_i / pair_j / common_out is NULL", fn);
    GAE_REQUIRE(nw == 0 || m == 0 || wsum_out, GAE_E_NULL, "%s: wsum_out is NULL", fn);
    GAE_REQUIRE(nw == 0 || n == 0 || W, GAE_E_NULL, "%s: W is NULL", fn);
    if (m == 0) return GAE_OK;
    PairArgs a;
    a.g = Csr{indptr, indices, int(n), nnz};
    a.pi = pair_i; a.pj = pair_j; a.m = m;
    a.W = W; a.nw = int(nw);
    a.common = common_out; a.wsum = wsum_out; a.status = status;
    hipLaunchKernelGGL(neighbour_pairs_kernel, dim3(unsigned(cdiv(m * kGroup, 256))), dim3(256), 0, gae::as_stream(stream), a);
    GAE_CHECK_LAUNCH("neighbour_pairs_kernel");
    return GAE_OK;
}

extern "C" int64_t gae_neighbour_topk_workspace_bytes(int64_t n, int64_t m)
{
    if (const int rc = check_topk_shape("gae_neighbour_topk_workspace_bytes", n, m)) return rc;
    return carve_topk(m, nullptr).need;
}

extern "C" int gae_neighbour_topk(const int32_t *indptr, const int32_t *indices, int64_t n, int64_t nnz, const int32_t *rows,
                                  int64_t m, int64_t k, int kind, const int64_t *w, int64_t ldw, const int32_t *deg, int flags,
                                  int64_t table_slots, int32_t *index_out, int32_t *common_out, int64_t *wsum_out,
                                  int64_t *status, void *workspace, int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_neighbour_topk";
    if (const int rc = check_graph(fn, indptr, indices, n, nnz)) return rc;
    if (const int rc = check_topk_shape(fn, n, m)) return rc;
    GAE_REQUIRE(k >= 1 && k <= kMaxK, GAE_E_RANGE, "%s: k = %lld outside 1..%d", fn, (long long)k, kMaxK);
    GAE_REQUIRE(kind == GAE_NEIGHBOUR_CN || kind == GAE_NEIGHBOUR_JACCARD || kind == GAE_NEIGHBOUR_AA || kind == GAE_NEIGHBOUR_RA,
                GAE_E_RANGE, "%s: kind = %d (cn 0, jaccard 1, aa 2, ra 3; pa is not a local score)", fn, kind);
    GAE_REQUIRE((flags & ~GAE_NEIGHBOUR_EXCLUDE_EDGES) == 0, GAE_E_RANGE, "%s: unknown flag bits 0x%x", fn, flags);
    if (table_slots == 0) table_slots = GAE_NEIGHBOUR_TABLE_SLOTS;
    GAE_REQUIRE(slots_taken(table_slots), GAE_E_RANGE, "%s: table_slots = %lld is not 0 or a power of two in 64..%d", fn,
                (long long)table_slots, kMaxSlots);
    const bool weighted = kind == GAE_NEIGHBOUR_AA || kind == GAE_NEIGHBOUR_RA;
    GAE_REQUIRE(!weighted || ldw >= 1, GAE_E_SIZE, "%s: ldw = %lld below 1", fn, (long long)ldw);
    GAE_REQUIRE(status, GAE_E_NULL, "%s: status is NULL", fn);
    GAE_REQUIRE(m == 0 || (index_out && common_out && wsum_out), GAE_E_NULL, "%s: index_out / common_out / wsum_out is NULL", fn);
    GAE_REQUIRE(n == 0 || deg, GAE_E_NULL, "%s: deg is NULL", fn);
    GAE_REQUIRE(!weighted || n == 0 || w, GAE_E_NULL, "%s: w is NULL for kind %d", fn, kind);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    const TopkPlan p = carve_topk(m, workspace);
    GAE_REQUIRE(workspace_bytes >= p.need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)p.need);
    if (m == 0) return GAE_OK;

    TopkArgs a;
    a.g = Csr{indptr, indices, int(n), nnz};
    a.rows = rows; a.m = m;
    a.k = int(k); a.kind = kind; a.exclude = (flags & GAE_NEIGHBOUR_EXCLUDE_EDGES) ? 1 : 0;
    a.w = weighted ? w : nullptr; a.ldw = ldw;
    a.deg = deg;
    a.slots = int(table_slots);
    a.log_slots = 0;
    while ((1 << a.log_slots) < a.slots) ++a.log_slots;
    a.index_out = index_out; a.common_out = common_out; a.wsum_out = wsum_out;
    a.status = status;
    a.counts = p.counts; a.short_list = p.short_list; a.long_list = p.long_list;
    hipStream_t st = gae::as_stream(stream);
    GAE_HIP(hipMemsetAsync(p.counts, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(neighbour_plan_kernel, dim3(unsigned(cdiv(m, 256))), dim3(256), 0, st, a);
    GAE_CHECK_LAUNCH("neighbour_plan_kernel");
    // the lists' lengths stay on the device: both grids cover m rows and a block beyond its list returns at once
    if (const int rc = gae::launch_lds<&neighbour_topk_short_kernel>("neighbour_topk_short_kernel", m, 64,
                                                                     size_t(lds_bytes(a.slots, false)), st, a))
        return rc;
    return gae::launch_lds<&neighbour_topk_long_kernel>("neighbour_topk_long_kernel", m, kLongThreads,
                                                        size_t(lds_bytes(a.slots, true)), st, a);
}
