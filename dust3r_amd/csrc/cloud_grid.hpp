// dust3r_amd -- what cloud_nn.hip (the grid, the distance statistics), cloud_knn.hip (the search on the grid), cloud_icp.hip (the
// registration's sums) and cloud_cluster.hip (the density clustering) share: the layout of the grid's workspace, the checks of the cell
// size and the radius, the 1 x n shape table, THE WALK of a point's padded cell range over the grid (GridWalk / cloud_walk: the one text
// that the search and the three clustering kernels run, and that the exactness argument of DESIGN.md 4.12 rests on), the (d2, index) pair
// as one 64-bit key, and the ordered fp64 / int64 sum: the workgroup's sum (reduce.hpp's reduction, whose header states the order), the
// final kernel over the per-workgroup partials and the partials' layout. As in fuse_grid.hpp every kernel is static, so each file launches its own copy.
#pragma once
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"

namespace d3r {
namespace cloud {

using namespace d3r::fuse;

constexpr int QT = 256;                 // threads of the per-point kernels

static __global__ __launch_bounds__(64) void cloud_shape_kernel(int* __restrict__ shape, int n) {
    if (threadIdx.x == 0) {
        shape[0] = 1;
        shape[1] = n;
    }
}

// the next fp32 above x (nextafterf(x, +inf)): +inf and NaN stay
D3R_DEV float next_up(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x);
    if (x != x || u == 0x7F800000u) return x;
    if ((u & 0x7FFFFFFFu) == 0u) return __builtin_bit_cast(float, 1u);
    return __builtin_bit_cast(float, (u & 0x80000000u) ? u - 1u : u + 1u);
}
D3R_DEV float next_down(float x) { return -next_up(-x); }

// floorf((x - lo_c) / cell), before the clamp
D3R_DEV float axis_f(float x, const KeyParams& k, int c) { return floorf(__fdiv_rn(__fsub_rn(x, k.lo[c]), k.voxel)); }

struct CloudWorkspace {
    int* shape;             // [4]: the reference cloud as a view of 1 x n_ref, the query cloud as one of 1 x n_query
    FuseWorkspace ref;      // stages 1-3 on the reference cloud; its n_dev = (valid points N, cells M) stays for the queries
    float4* pts4;           // [n_ref]: the valid reference points in cell order, w = the original index
    uint64_t* cell_key;     // [n_ref]
    int* cell_start;        // [n_ref + 1]
    FuseWorkspace qry;      // stages 1-2 on the queries
    uint8_t* mask;          // [n_query]: only_unresolved
    size_t bytes;
};

static inline CloudWorkspace cloud_workspace(void* base, int n_ref, int n_query) {
    CloudWorkspace w;
    Carver c(base);
    w.shape = c.take<int>(4);
    w.ref = fuse_workspace(c.take<char>(0), 1, n_ref, n_ref);
    c.bytes += w.ref.bytes;
    w.pts4 = c.take<float4>(n_ref);
    w.cell_key = c.take<uint64_t>(n_ref);
    w.cell_start = c.take<int>((size_t)n_ref + 1);
    w.qry = fuse_workspace(c.take<char>(0), 1, n_query, n_query);
    c.bytes += w.qry.bytes;
    w.mask = c.take<uint8_t>(n_query);
    w.bytes = c.bytes;
    return w;
}

static inline bool cloud_cell_ok(float cell) { return cell > 0.f && cell <= 3.0e38f; }
// r r must be a normal fp32 number: a subnormal or zero r2 accepts d2 = 0 from coordinates far beyond r (their squares flush), an infinite
// one accepts every point -- in both cases d2 <= r2 no longer bounds the coordinates by r', which is what the cell range rests on
static inline bool cloud_radius_ok(float r) {
    const float r2 = r * r;                                             // host code of files built without contraction: one fp32 product
    return r > 0.f && r2 >= 1.17549435e-38f && r2 <= 3.4028234e38f;
}
static inline int cloud_blocks(long long n) { return blocks_of(tiles_of(n, QT), MAX_BLOCKS); }

// ---- the walk ----------------------------------------------------------------------------------------------------------------------------
constexpr int NO_INDEX = 0x7FFFFFFF;    // the index of an empty slot: above every real one, so (inf, NO_INDEX) sorts last

// The pair (d2, g) as one 64-bit key, d2's bits above g: d2 is a sum of squares, so +0 <= d2 <= +inf and never NaN for finite coordinates,
// and the bits of such floats order as unsigned integers; g >= 0. Lexicographic (d2, g) order is the unsigned order of the keys: one
// comparison per candidate. The empty slot (+inf, NO_INDEX) is above every pair a walk accepts (d2 <= r2 < inf).
D3R_DEV uint64_t pair_key(float d2, int g) { return ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)g; }

struct GridWalk {
    KeyParams key;
    float r;
    const float4* pts4;                 // the grid: the valid points in cell order, w = the original index
    const uint64_t* cell_key;
    const int* cell_start;
    const int* n_dev;                   // [2]: the valid points N, the cells M
    int cap;
};

// The walk for the point (ax, ay, az) over the M cells: per axis the cells from q(next_down(a - r')) to q(next_up(a + r')), r' = r (1 +
// 2^-10); per (z, y) row one binary search and one run of points. f(i, d2, v) for EVERY looked-at point i (sorted position), d2 in fp32 with
// every operation rounded on its own -- the caller tests d2 <= r2. Returns the distances evaluated.
template <class F>
D3R_DEV int cloud_walk(const GridWalk& a, int M, float ax, float ay, float az, F&& f) {
    const float rp = __fmul_rn(a.r, 1.0009765625f);
    const float pa[3] = {ax, ay, az};
    int c0[3], c1[3];
    bool outside = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lo = next_down(__fsub_rn(pa[c], rp)), hi = next_up(__fadd_rn(pa[c], rp));
        // every grid point has 0 <= floorf(.) <= qmax (lo = the bounds' minimum, bits from their extent) and floorf(.) is monotone: an
        // interval that ends below cell 0 or starts above the last cell holds none
        outside = outside || axis_f(hi, a.key, c) < 0.f || axis_f(lo, a.key, c) > (float)a.key.qmax[c];
        c0[c] = axis_q(lo, a.key, c);
        c1[c] = axis_q(hi, a.key, c);
    }
    if (outside) return 0;
    int evals = 0, from = 0;                                               // the rows come in ascending key order: each search starts where the last ended
    for (int z = c0[2]; z <= c1[2]; ++z) {
        for (int y = c0[1]; y <= c1[1]; ++y) {
            const uint64_t row = ((uint64_t)y << a.key.shift[1]) | ((uint64_t)z << a.key.shift[2]);
            const uint64_t k_lo = row | (uint64_t)c0[0], k_hi = row | (uint64_t)c1[0];
            int l = from, h = M;                                           // the first cell with key >= k_lo
            while (l < h) {
                const int m = l + ((h - l) >> 1);
                if (a.cell_key[m] < k_lo) l = m + 1; else h = m;
            }
            int j = l;
            while (j < M && a.cell_key[j] <= k_hi) ++j;                   // at most c1 - c0 + 1 cells: one run of points
            from = j;
            if (j == l) continue;
            const int s = a.cell_start[l], e = a.cell_start[j];
            for (int i = s; i < e; ++i) {
                const float4 v = a.pts4[i];
                const float dx = __fsub_rn(ax, v.x), dy = __fsub_rn(ay, v.y), dz = __fsub_rn(az, v.z);
                f(i, dist2(dx, dy, dz), v);
            }
            evals += e - s;
        }
    }
    return evals;
}

// ---- the ordered sum: ND doubles and NI int64s per thread -> per workgroup -> one row -------------------------------------------------------
constexpr int SUM_PARTS = 1024;         // grid cap of a pass that leaves partials = the rows the final kernel reads

// The workgroup's totals of sd / si, column k written to out_d[k] / out_i[k] by thread k: reduce.hpp's workgroup reduction of both types
// behind one barrier. A fixed shape: the same bytes whatever the run. Once per kernel (it owns its LDS).
template <int ND, int NI>
D3R_DEV void cloud_block_sum(double (&sd)[ND], long long (&si)[NI], double* out_d, long long* out_i) {
    static_assert(ND <= QT && NI <= QT, "one thread per column");
    __shared__ double lds_d[QT / 64 * ND];
    __shared__ long long lds_i[QT / 64 * NI];
    block_reduce_stage(si, lds_i, Sum());                                // the integers first: after the 18 fp64 columns, cloud_icp_sums_kernel<0> needs 82 VGPRs for 80
    block_reduce_stage(sd, lds_d, Sum());
    __syncthreads();
    if (threadIdx.x < ND) out_d[threadIdx.x] = block_reduce_column<QT, ND>(lds_d, threadIdx.x, Sum());
    if (threadIdx.x < NI) out_i[threadIdx.x] = block_reduce_column<QT, NI>(lds_i, threadIdx.x, Sum());
}

// one workgroup adds the partials: thread t the rows t, t + QT, ... in index order, then the workgroup's sum
template <int ND, int NI>
static __global__ __launch_bounds__(QT) void cloud_sums_final_kernel(int n_parts, const double* __restrict__ part_d, const long long* __restrict__ part_i,
                                                                    long long* __restrict__ counts_out, double* __restrict__ sums_out) {
    double sd[ND];
    long long si[NI];
#pragma unroll
    for (int k = 0; k < ND; ++k) sd[k] = 0.0;
#pragma unroll
    for (int k = 0; k < NI; ++k) si[k] = 0;
    for (int b = threadIdx.x; b < n_parts; b += QT) {
#pragma unroll
        for (int k = 0; k < ND; ++k) sd[k] += part_d[(size_t)b * ND + k];
#pragma unroll
        for (int k = 0; k < NI; ++k) si[k] += part_i[(size_t)b * NI + k];
    }
    cloud_block_sum<ND, NI>(sd, si, sums_out, counts_out);
}

struct SumParts {
    int parts;              // the workgroups of the pass over n rows
    double* d;              // [parts][nd]
    long long* i;           // [parts][ni]
    size_t bytes;
};

static inline SumParts cloud_sum_parts(void* base, int n, int nd, int ni) {
    SumParts p;
    Carver c(base);
    p.parts = std::min(cloud_blocks(n), SUM_PARTS);
    p.d = c.take<double>((size_t)p.parts * nd);
    p.i = c.take<long long>((size_t)p.parts * ni);
    p.bytes = c.bytes;
    return p;
}

}  // namespace cloud
}  // namespace d3r
