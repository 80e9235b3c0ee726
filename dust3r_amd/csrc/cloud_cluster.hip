// dust3r_amd -- density clustering of a cloud (DBSCAN; new, the reference has none): d3r_cloud_cluster on the grid of d3r_cloud_grid_build
// (cloud_nn.hip, cloud_grid.hpp), built on the cloud itself (dust3r_amd/cloud_metrics.py cluster_points, viz.FusedCloud.cluster /
// keep_clusters). The contract does not mention the grid (include/dust3r_hip.h): neighbours are the valid points with fp32 d2 <= eps2, the
// point itself included; core points have min_points of them; clusters are the connected components of the core graph, rooted at their
// lowest index; a border point goes to the core neighbour of smallest (d2, index); clusters are numbered by decreasing size, ties by root.
// The grid only limits which points are LOOKED AT: every walk is cloud_grid.hpp's cloud_walk, the search's own.
//   cluster_init_kernel       every point: parent = itself, no neighbours, not core
//   cluster_count_kernel      one thread per valid point in cell order walks its range: n_neighbors, the core flag
//   cluster_union_kernel      a core point walks again: every core neighbour of lower index is united with it, lock-free (below)
//   cluster_flatten_kernel    root of every core point; -1 for the others
//   cluster_border_kernel     a valid non-core point walks: the root of the core neighbour of minimal (d2 bits, index) key
//   fuse_flag_kernel<ROOTS>   the labelled points compacted as (root, point), fuse_sort_pairs by root, fuse_segment_heads: one segment per
//   cluster_keys_kernel       cluster (fuse_grid.hpp); (n - size, cluster) sorted stably by the first: decreasing size, equal sizes keep ascending roots
//   cluster_rank_kernel / cluster_label_kernel   sizes in rank order, root -> rank, rank -> labels
// THE UNION-FIND is the only place in the cloud code where workgroups touch the same words. parent[x] <= x always, == x exactly for a
// root, and it is only ever lowered (atomicCAS on a root, atomicMin when a find halves a path) to a member of x's own component. No
// thread waits for another: find follows a strictly decreasing chain, and a failed CAS hands back the lower parent someone else wrote,
// from which the thread goes on. Every tree's root is its minimum (a larger root is hooked under a smaller index of the other tree), and
// after all edges are in, a component is one tree: the flattened roots do not depend on the interleaving. No scratch: lists are walked.
#include "../../include/dust3r_hip.h"
#include "common.hpp"
#include "scene_common.hpp"
#include "fuse_grid.hpp"
#include "cloud_grid.hpp"

namespace d3r {
namespace cloud {

__global__ __launch_bounds__(QT) void cluster_init_kernel(int n, int* __restrict__ parent, int* __restrict__ n_neighbors, uint8_t* __restrict__ core) {
    for (long long g = (long long)blockIdx.x * QT + threadIdx.x; g < n; g += (long long)gridDim.x * QT) {
        parent[g] = (int)g;
        n_neighbors[g] = 0;
        core[g] = 0;
    }
}

__global__ __launch_bounds__(QT) void cluster_count_kernel(const GridWalk a, int min_points, int* __restrict__ n_neighbors, uint8_t* __restrict__ core,
                                                          uint8_t* __restrict__ core_sorted, int* __restrict__ evals) {
    const int N = count_of(a.n_dev, a.cap), M = count_of(a.n_dev + 1, a.cap);
    const float r2 = __fmul_rn(a.r, a.r);
    for (long long t = (long long)blockIdx.x * QT + threadIdx.x; t < N; t += (long long)gridDim.x * QT) {
        const float4 p = a.pts4[t];
        const int g = __float_as_int(p.w);
        int cnt = 0;
        const int ev = cloud_walk(a, M, p.x, p.y, p.z, [&](int, float d2, const float4&) { cnt += d2 <= r2; });
        const bool is_core = cnt >= min_points;
        n_neighbors[g] = cnt;
        core[g] = is_core;
        core_sorted[t] = is_core;
        if (evals) evals[g] += ev;
    }
}

// ---- lock-free union-find on original indices ----------------------------------------------------------------------------------------------
D3R_DEV int parent_load(const int* parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as far as this thread can see it: every step goes to a strictly lower index, so at most x steps. A path is halved on
// the way (atomicMin: parent only ever goes down). A stale value is one parent[x] once held, hence still an ancestor: it costs steps only.
D3R_DEV int cluster_find(int* parent, int x) {
    int p = parent_load(parent, x);
    while (p < x) {
        const int gp = parent_load(parent, p);
        if (gp < p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

// One tree of the two: the larger root is hooked under the smaller index. The CAS succeeds only on a true root; when it fails, `old` is
// the lower parent someone else gave a, and the search goes on from there: max(a, b) falls in every round.
D3R_DEV void cluster_unite(int* parent, int a, int b) {
    a = cluster_find(parent, a);
    b = cluster_find(parent, b);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicCAS(parent + a, a, b);
        if (old >= a) break;                                               // old == a: hooked (old > a cannot happen: parent[a] <= a)
        a = cluster_find(parent, old);
        b = cluster_find(parent, b);
    }
}

__global__ __launch_bounds__(QT) void cluster_union_kernel(const GridWalk a, const uint8_t* __restrict__ core_sorted, int* parent) {
    const int N = count_of(a.n_dev, a.cap), M = count_of(a.n_dev + 1, a.cap);
    const float r2 = __fmul_rn(a.r, a.r);
    for (long long t = (long long)blockIdx.x * QT + threadIdx.x; t < N; t += (long long)gridDim.x * QT) {
        if (!core_sorted[t]) continue;
        const float4 p = a.pts4[t];
        const int g = __float_as_int(p.w);
        cloud_walk(a, M, p.x, p.y, p.z, [&](int i, float d2, const float4& v) {
            const int h = __float_as_int(v.w);
            if (d2 <= r2 && h < g && core_sorted[i]) cluster_unite(parent, g, h);
        });
    }
}

// after the union kernel's end every parent is final and visible: plain loads
__global__ __launch_bounds__(QT) void cluster_flatten_kernel(int n, const int* __restrict__ parent, const uint8_t* __restrict__ core, int* __restrict__ root) {
    for (long long g = (long long)blockIdx.x * QT + threadIdx.x; g < n; g += (long long)gridDim.x * QT) {
        int x = -1;
        if (core[g]) {
            x = (int)g;
            int p = parent[x];
            while (p < x) {
                x = p;
                p = parent[x];
            }
        }
        root[g] = x;
    }
}

// root is read at core points and written at non-core points only
__global__ __launch_bounds__(QT) void cluster_border_kernel(const GridWalk a, const uint8_t* __restrict__ core_sorted, int* root) {
    const int N = count_of(a.n_dev, a.cap), M = count_of(a.n_dev + 1, a.cap);
    const float r2 = __fmul_rn(a.r, a.r);
    for (long long t = (long long)blockIdx.x * QT + threadIdx.x; t < N; t += (long long)gridDim.x * QT) {
        if (core_sorted[t]) continue;
        const float4 p = a.pts4[t];
        const uint64_t none = pair_key(__builtin_huge_valf(), NO_INDEX);
        uint64_t best = none;
        cloud_walk(a, M, p.x, p.y, p.z, [&](int i, float d2, const float4& v) {
            const uint64_t cand = pair_key(d2, __float_as_int(v.w));
            if (d2 <= r2 && core_sorted[i] && cand < best) best = cand;
        });
        if (best != none) root[__float_as_int(p.w)] = root[(int)(uint32_t)best];
    }
}

// ---- numbering -----------------------------------------------------------------------------------------------------------------------------
// cluster c = segment c of the pairs sorted by root: the key n - size (0 <= key < n), so an ascending stable sort gives decreasing sizes
__global__ __launch_bounds__(QT) void cluster_keys_kernel(int n, const int* __restrict__ starts, const int* __restrict__ n_dev, uint64_t* __restrict__ ckeys,
                                                         int* __restrict__ cidx) {
    const int L = count_of(n_dev, n), Cn = count_of(n_dev + 1, n);
    for (long long c = (long long)blockIdx.x * QT + threadIdx.x; c < Cn; c += (long long)gridDim.x * QT) {
        const int s = starts[c], e = c + 1 < Cn ? starts[c + 1] : L;
        ckeys[c] = (uint64_t)(n - (e - s));
        cidx[c] = (int)c;
    }
}

// rank r: its size, and rank_of[root] = r (rank_of is the parent array, done with)
__global__ __launch_bounds__(QT) void cluster_rank_kernel(int n, const uint64_t* __restrict__ ckeys, const int* __restrict__ cidx, const int* __restrict__ starts,
                                                         const uint64_t* __restrict__ sorted_roots, const int* __restrict__ n_dev, int* __restrict__ sizes,
                                                         int* __restrict__ rank_of, int* __restrict__ n_clusters) {
    const int Cn = count_of(n_dev + 1, n);
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_clusters = Cn;
    for (long long r = (long long)blockIdx.x * QT + threadIdx.x; r < Cn; r += (long long)gridDim.x * QT) {
        const int c = min(max(cidx[r], 0), Cn - 1);
        const int rt = (int)sorted_roots[starts[c]];
        sizes[r] = n - (int)ckeys[r];
        if (rt >= 0 && rt < n) rank_of[rt] = (int)r;
    }
}

__global__ __launch_bounds__(QT) void cluster_label_kernel(int n, const int* __restrict__ root, const int* __restrict__ rank_of, int* __restrict__ labels) {
    for (long long g = (long long)blockIdx.x * QT + threadIdx.x; g < n; g += (long long)gridDim.x * QT) {
        const int rt = root[g];
        labels[g] = rt >= 0 ? rank_of[rt] : -1;
    }
}

struct ClusterWorkspace {
    FuseWorkspace f;        // the (root, point) pairs, their sort and segment heads
    int* parent;            // [n]; after the flattening rank_of
    int* root;              // [n]
    uint8_t* core_sorted;   // [n]: the core flag by sorted position
    uint64_t* ckeys[2];     // [n] each: the clusters' sort
    int* cidx[2];
    size_t bytes;
};

static inline ClusterWorkspace cluster_workspace(void* base, int n) {
    ClusterWorkspace w;
    Carver c(base);
    w.f = fuse_workspace(c.take<char>(0), 1, n, n);
    c.bytes += w.f.bytes;
    w.parent = c.take<int>(n);
    w.root = c.take<int>(n);
    w.core_sorted = c.take<uint8_t>(n);
    w.ckeys[0] = c.take<uint64_t>(n);
    w.ckeys[1] = c.take<uint64_t>(n);
    w.cidx[0] = c.take<int>(n);
    w.cidx[1] = c.take<int>(n);
    w.bytes = c.bytes;
    return w;
}

}  // namespace cloud
}  // namespace d3r

using namespace d3r::cloud;

extern "C" size_t d3r_cloud_cluster_workspace_bytes(int n) {
    if (!fuse_shape_ok(1, n, n)) return 0;
    return cluster_workspace(nullptr, n).bytes;
}

extern "C" int d3r_cloud_cluster(int n, float eps, int min_points, const float* lo, float cell, const int* bits, int* labels_out, int* sizes_out,
                                 int* n_clusters_out, int* n_neighbors_out, uint8_t* core_out, int* evals, void* const* stage_events, void* grid_workspace,
                                 void* workspace, void* stream) {
    if (!fuse_shape_ok(1, n, n) || !lo || !bits || !labels_out || !sizes_out || !n_clusters_out || !n_neighbors_out || !core_out || !grid_workspace ||
        !workspace || !cloud_radius_ok(eps) || !cloud_cell_ok(cell) || min_points < 1)
        return D3R_ERR_INVALID;
    GridWalk a;
    int total_bits = 0;
    if (!fuse_key_params(lo, cell, bits, &a.key, &total_bits)) return D3R_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const CloudWorkspace g = cloud_workspace(grid_workspace, n, 1);
    const ClusterWorkspace w = cluster_workspace(workspace, n);
    a.r = eps; a.pts4 = g.pts4; a.cell_key = g.cell_key; a.cell_start = g.cell_start; a.n_dev = g.ref.n_dev; a.cap = n;
    const dim3 grid(cloud_blocks(n)), block(QT);
    auto mark = [&](int k) {
        if (stage_events && stage_events[k]) (void)hipEventRecord((hipEvent_t)stage_events[k], st);
    };
    // neighbours and core points
    hipLaunchKernelGGL(cluster_init_kernel, grid, block, 0, st, n, w.parent, n_neighbors_out, core_out);
    hipLaunchKernelGGL(cluster_count_kernel, grid, block, 0, st, a, min_points, n_neighbors_out, core_out, w.core_sorted, evals);
    mark(0);
    // components of the core graph
    hipLaunchKernelGGL(cluster_union_kernel, grid, block, 0, st, a, w.core_sorted, w.parent);
    hipLaunchKernelGGL(cluster_flatten_kernel, grid, block, 0, st, n, w.parent, core_out, w.root);
    mark(1);
    hipLaunchKernelGGL(cluster_border_kernel, grid, block, 0, st, a, w.core_sorted, w.root);
    mark(2);
    // numbering: (root, point) of the labelled points, sorted by root; one segment per cluster
    const long long tiles = d3r::tiles_of(n, NT);
    const dim3 tile_grid(d3r::blocks_of(tiles, MAX_BLOCKS));
    FlagArgs fa = {};                                                      // ROOTS and HEADS read root, n_dev, cap and the sorted keys only
    fa.root = w.root; fa.n_dev = w.f.n_dev; fa.cap = n;
    hipLaunchKernelGGL((fuse_flag_kernel<ROOTS, false>), tile_grid, dim3(NT), 0, st, fa, tiles, w.f.tile_cnt, w.f.keys[0], w.f.idx[0]);
    hipLaunchKernelGGL(fuse_scan_kernel, dim3(1), dim3(NT), 0, st, w.f.tile_cnt, (int)tiles, w.f.n_dev);
    hipLaunchKernelGGL((fuse_flag_kernel<ROOTS, true>), tile_grid, dim3(NT), 0, st, fa, tiles, w.f.tile_cnt, w.f.keys[0], w.f.idx[0]);
    const int index_bits = bit_length((unsigned)(n - 1));
    const int cur = fuse_sort_pairs(w.f.keys, w.f.idx, w.f.hist, w.f.n_dev, n, index_bits, 0, st);
    const int* starts = fuse_segment_heads(fa, w.f, cur, n, st);
    // the clusters by (n - size), stable: equal sizes stay in ascending root order
    hipLaunchKernelGGL(cluster_keys_kernel, grid, block, 0, st, n, starts, w.f.n_dev, w.ckeys[0], w.cidx[0]);
    const int ccur = fuse_sort_pairs(w.ckeys, w.cidx, w.f.hist, w.f.n_dev + 1, n, index_bits, 0, st);
    hipLaunchKernelGGL(cluster_rank_kernel, grid, block, 0, st, n, w.ckeys[ccur], w.cidx[ccur], starts, w.f.keys[cur], w.f.n_dev, sizes_out, w.parent,
                       n_clusters_out);
    hipLaunchKernelGGL(cluster_label_kernel, grid, block, 0, st, n, w.root, w.parent, labels_out);
    mark(3);
    return rc_of(hipGetLastError());
}
