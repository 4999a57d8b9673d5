// K33: circular (Morgan / Weisfeiler-Lehman) fingerprints of the member graphs of a resident molecule set
// (ops.fingerprint_graphs, DeviceGraphDataset.fingerprints).  The contract -- the hash, the radius rule, emission, the
// defensive rules -- is the comment of gae_fingerprint_graphs in include/gae_hip_experimental.h.
//
// Launches (ordinary ones; integer atomics only, no float anywhere):
//   zero     the B output rows, columns [0, width) only: the caller's pad columns are not touched
//   radius r = 0 .. R, one launch each: launch boundaries are the only synchronisation.  One wave per output slot, four
//            slots per block; the wave walks its graph's atoms in strides of 64, so a graph of any size is taken and the
//            work is that of the LISTED graphs.  Launch 0 hashes the atom's feature row; launch r reads id_{r-1} of the
//            atom and of its CSR row from the workspace array (r - 1) & 1 and writes id_r into array r & 1 (both uint64
//            [N], indexed by global node id).  A graph listed twice is walked twice and stores the same ids twice.
//            Every (atom, r) emits slot id mod n_bits into the slot's output row: atomicOr of the bit, or atomicAdd of
//            one to the count.  Both are exact and order-free, so the rows have the same bits run to run.
#include "common.h"

namespace {

constexpr int kMaxRadius = 8;
constexpr int kSlotsPerBlock = 4;
constexpr uint64_t kGold = 0x9e3779b97f4a7c15ull;

struct FpArgs {
    const int64_t *graph_ptr;
    int64_t G, N, E;
    const int32_t *indptr, *indices;
    const void *feat;
    int u8;
    int64_t ldf;
    int F;
    const int64_t *graph_ids;
    int64_t B;
    int r;                                 // the radius of this launch
    uint32_t mask;                         // n_bits - 1
    int counts;
    int32_t *out;
    int64_t ldo;
    const uint64_t *prev;                  // id_{r-1} [N]
    uint64_t *next;                        // id_r [N]
};

// the splitmix64 finaliser
__host__ __device__ __forceinline__ uint64_t mix(uint64_t x)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

// the fp32 bit pattern of the integer v in 0 .. 255, by integer steps alone
__device__ __forceinline__ uint32_t f32_bits_of_u8(uint32_t v)
{
    if (v == 0) return 0u;
    const int e = 31 - __clz(int(v));
    return (uint32_t(127 + e) << 23) | ((v << (23 - e)) & 0x7fffffu);
}

__global__ __launch_bounds__(256) void fingerprint_zero_kernel(int32_t *out, int64_t ldo, int64_t B, int width)
{
    const int64_t total = B * width;
    for (int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x; t < total; t += int64_t(gridDim.x) * 256)
        out[(t / width) * ldo + t % width] = 0;
}

__global__ __launch_bounds__(64 * kSlotsPerBlock) void fingerprint_kernel(const FpArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t slot = int64_t(blockIdx.x) * kSlotsPerBlock + (threadIdx.x >> 6);
    if (slot >= a.B) return;
    // the slot's graph: a bad id or node range leaves the (zeroed) row as it is
    const int64_t gid = a.graph_ids ? a.graph_ids[slot] : slot;
    if (gid < 0 || gid >= a.G) return;
    const int64_t r0 = a.graph_ptr[gid], r1 = a.graph_ptr[gid + 1];
    if (r0 < 0 || r1 < r0 || r1 > a.N) return;
    int32_t *row = a.out + slot * a.ldo;
    for (int64_t v = r0 + lane; v < r1; v += 64) {
        uint64_t id;
        if (a.r == 0) {
            uint64_t h = kGold;
            if (a.u8) {
                const uint8_t *p = static_cast<const uint8_t *>(a.feat) + v * a.ldf;
                for (int f = 0; f < a.F; ++f) h = mix(h ^ uint64_t(f32_bits_of_u8(p[f])));
            } else {
                const uint32_t *p = static_cast<const uint32_t *>(a.feat) + v * a.ldf;
                for (int f = 0; f < a.F; ++f) {
                    uint32_t b = p[f];
                    if (b == 0x80000000u) b = 0u;              // -0.0 hashes as +0.0
                    h = mix(h ^ uint64_t(b));
                }
            }
            id = h;
        } else {
            // a row pointer outside [0, E] reads as an empty row; a column outside the graph's own rows is skipped
            int64_t e0 = a.indptr[v], e1 = a.indptr[v + 1];
            if (e0 < 0 || e1 < e0 || e1 > a.E) e0 = e1 = 0;
            uint64_t sum = 0;
            for (int64_t e = e0; e < e1; ++e) {
                const int64_t c = a.indices[e];
                if (c >= r0 && c < r1) sum += mix(a.prev[c]);
            }
            id = mix(mix(a.prev[v] + uint64_t(a.r) * kGold) + sum);
        }
        a.next[v] = id;
        const uint32_t s = uint32_t(id) & a.mask;
        if (a.counts) atomicAdd(row + s, 1);
        else atomicOr(reinterpret_cast<unsigned *>(row) + (s >> 5), 1u << (s & 31));
    }
}

bool n_bits_taken(int64_t n_bits) { return n_bits >= 64 && n_bits <= 2048 && (n_bits & (n_bits - 1)) == 0; }

} // namespace

extern "C" int64_t gae_fingerprint_workspace_bytes(int64_t n_nodes)
{
    GAE_REQUIRE(n_nodes >= 0 && n_nodes < (int64_t(1) << 31), GAE_E_SIZE,
                "gae_fingerprint_workspace_bytes: n_nodes = %lld outside 0 .. 2^31 - 1", (long long)n_nodes);
    gae::Carver c(nullptr);
    c.take<uint64_t>(n_nodes);
    c.take<uint64_t>(n_nodes);
    return c.bytes() + 256;
}

extern "C" int gae_fingerprint_graphs(const int64_t *graph_ptr, int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                                      const int32_t *indptr, const int32_t *indices, const void *feat, int feat_dtype,
                                      int64_t ldf, int64_t f_in, const int64_t *graph_ids, int64_t n_out, int radius,
                                      int64_t n_bits, int counts, int32_t *out, int64_t ldo, void *workspace,
                                      int64_t workspace_bytes, void *stream)
{
    const char *fn = "gae_fingerprint_graphs";
    GAE_REQUIRE(radius >= 0 && radius <= kMaxRadius, GAE_E_RANGE, "%s: radius = %d outside 0..%d", fn, radius, kMaxRadius);
    GAE_REQUIRE(n_bits_taken(n_bits), GAE_E_RANGE, "%s: n_bits = %lld is not a power of two in 64..2048", fn,
                (long long)n_bits);
    GAE_REQUIRE(counts == 0 || counts == 1, GAE_E_RANGE, "%s: counts = %d (0 = bits, 1 = counts)", fn, counts);
    GAE_REQUIRE(n_graphs >= 0 && n_nodes >= 0 && n_edges >= 0 && n_out >= 0, GAE_E_SIZE,
                "%s: negative n_graphs = %lld, n_nodes = %lld, n_edges = %lld or n_out = %lld", fn, (long long)n_graphs,
                (long long)n_nodes, (long long)n_edges, (long long)n_out);
    GAE_REQUIRE(n_nodes < (int64_t(1) << 31) && n_edges < (int64_t(1) << 31), GAE_E_SIZE,
                "%s: n_nodes = %lld or n_edges = %lld beyond the int32 CSR", fn, (long long)n_nodes, (long long)n_edges);
    GAE_REQUIRE(f_in >= 1 && f_in < (int64_t(1) << 31), GAE_E_RANGE, "%s: feature width f_in = %lld below 1", fn,
                (long long)f_in);
    GAE_REQUIRE(feat_dtype == GAE_F32 || feat_dtype == GAE_U8, GAE_E_DTYPE, "%s: feature dtype %d (GAE_F32 or GAE_U8)",
                fn, feat_dtype);
    const int width = int(counts ? n_bits : n_bits / 32);
    GAE_REQUIRE(ldf >= f_in && ldo >= width, GAE_E_SIZE,
                "%s: leading dimension too small (ldf %lld < f_in = %lld or ldo %lld < %d)", fn, (long long)ldf,
                (long long)f_in, (long long)ldo, width);
    GAE_REQUIRE(graph_ptr, GAE_E_NULL, "%s: graph_ptr is NULL", fn);
    GAE_REQUIRE(n_nodes == 0 || (indptr && feat), GAE_E_NULL, "%s: indptr / feat is NULL", fn);
    GAE_REQUIRE(n_edges == 0 || indices, GAE_E_NULL, "%s: indices is NULL", fn);
    GAE_REQUIRE(n_out == 0 || out, GAE_E_NULL, "%s: out is NULL", fn);
    GAE_REQUIRE(workspace, GAE_E_NULL, "%s: workspace is NULL", fn);
    const int64_t need = gae_fingerprint_workspace_bytes(n_nodes);
    GAE_REQUIRE(workspace_bytes >= need, GAE_E_WORKSPACE, "%s: workspace of %lld bytes, %lld needed", fn,
                (long long)workspace_bytes, (long long)need);
    const int64_t blocks = gae::cdiv(n_out, kSlotsPerBlock);
    GAE_REQUIRE(blocks < (int64_t(1) << 31), GAE_E_SIZE, "%s: a grid of %lld blocks", fn, (long long)blocks);
    if (n_out == 0) return GAE_OK;

    gae::Carver c(workspace);
    uint64_t *ids[2];
    ids[0] = c.take<uint64_t>(n_nodes);
    ids[1] = c.take<uint64_t>(n_nodes);
    hipStream_t st = gae::as_stream(stream);
    const int64_t zero_blocks = gae::cdiv(n_out * width, 256);
    hipLaunchKernelGGL(fingerprint_zero_kernel, dim3(unsigned(zero_blocks < 65536 ? zero_blocks : 65536)), dim3(256), 0,
                       st, out, ldo, n_out, width);
    GAE_CHECK_LAUNCH("fingerprint_zero_kernel");
    FpArgs a;
    a.graph_ptr = graph_ptr; a.G = n_graphs; a.N = n_nodes; a.E = n_edges;
    a.indptr = indptr; a.indices = indices;
    a.feat = feat; a.u8 = feat_dtype == GAE_U8 ? 1 : 0; a.ldf = ldf; a.F = int(f_in);
    a.graph_ids = graph_ids; a.B = n_out;
    a.mask = uint32_t(n_bits - 1); a.counts = counts;
    a.out = out; a.ldo = ldo;
    for (int r = 0; r <= radius; ++r) {
        a.r = r;
        a.prev = ids[(r + 1) & 1];
        a.next = ids[r & 1];
        hipLaunchKernelGGL(fingerprint_kernel, dim3(unsigned(blocks)), dim3(64 * kSlotsPerBlock), 0, st, a);
        GAE_CHECK_LAUNCH("fingerprint_kernel");
    }
    return GAE_OK;
}
