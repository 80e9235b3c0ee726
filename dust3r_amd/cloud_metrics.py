"""Cloud-to-cloud metrics on the GPU (new; the reference's paper reports them, its code has none): accuracy, completeness, overall (Chamfer),
precision / recall / F-score at a distance, of one cloud against another -- csrc/cloud_nn.hip (the grid, the statistics) and
csrc/cloud_knn.hip (the search), C ABI `d3r_cloud_grid_build` / `d3r_cloud_nearest` / `d3r_cloud_distance_stats` (include/dust3r_hip.h).

    d2, idx = nearest_in_cloud(query, ref, max_dist)        # the truncated exact nearest neighbour of every query point
    m = cloud_metrics(pred, gt, max_dist, thresholds)       # the dict of the metrics

The nearest neighbour is DEFINED without a grid: for a query with three finite coordinates, the lowest index among the reference points
(with three finite coordinates) of minimal fp32 squared distance, when that minimum is <= max_dist^2 (fp32); else, and for a non-finite
query, idx = -1 and d2 = +inf. The kernels give what an fp32 brute force over all pairs gives, bit for bit ("Cloud metrics").
A uniform grid with cells as large as max_dist would make every query walk thousands of points when the clouds are much denser than
max_dist, so the search runs as a radius ladder: r_k = min(r_0 4^k, max_dist), each pass on a grid of cell r_k and only for the queries no
earlier pass resolved. A neighbour found within r_k is the global nearest and all its ties lie within r_k, so the ladder's result is the
single search's at max_dist.

    d2, idx = k_nearest(query, ref, k, max_dist)            # the k nearest, rows sorted by (d2, index): csrc/cloud_knn.hip, d3r_cloud_knn

The same grid and ladder carry the k nearest neighbours, and three consumers of their rows: `knn_mean_distances` with `outlier_threshold`
(statistical outlier removal), `cloud_normals` and `orient_normals`; viz.FusedCloud.estimate_normals / remove_outliers and
scene.fuse(normals=..., outliers=...) are built of them.

    reg = register_clouds(src, dst, max_dist)               # Sim(3) ICP of src onto dst: csrc/cloud_icp.hip, d3r_cloud_transform / d3r_cloud_icp_sums

The same nearest neighbour carries the registration of one cloud onto another: per iteration the source is moved by the
current similarity, every moved point finds its nearest reference point on grids that are built once per stage, one kernel gates the pairs
and reduces them to 18 (point to point) or 36 (point to plane) fp64 sums, and the host solves for the update in fp64.

    res = cluster_points(points, eps, min_points)           # DBSCAN: labels, sizes, n_neighbors, core: csrc/cloud_cluster.hip, d3r_cloud_cluster

On the same grid, built on the cloud itself with cells of eps: density clustering, defined without the grid and without any visiting
order; viz.FusedCloud.cluster / keep_clusters and scene.fuse(clusters=..., keep_largest=...) are built of it.

    res = global_registration(src, dst)                     # a coarse Sim(3) from nothing: csrc/cloud_features.hip

The similarity `register_clouds` starts from, when nobody has one: `grid_subsample` at a cell relative to each cloud's
own size, FPFH descriptors of the k nearest neighbours (`spfh_counts`, `fpfh_features`), exhaustive mutual matching in 33 dimensions
(`feature_nearest`, `match_features`) and a Sim(3) RANSAC over the matches (`sim3_ransac`); `register_clouds(..., init='global')` chains
the two.

    res = detect_planes(cloud, thr)                         # planes, their sizes, a plane label per point: csrc/cloud_planes.hip

Where the floor is, where the walls are, which way is up: a plane RANSAC over ALL points of the cloud (`plane_ransac`),
refits on the fp64 moments of the inliers (`plane_support`, `plane_from_moments`; together `segment_plane`), sequential extraction
(`detect_planes`), and on the host the ground among the planes and the motion that stands the scene on it (`ground_plane`,
`upright_similarity`); viz.FusedCloud.detect_planes / remove_planes / upright and scene.fuse(planes=..., upright=...) are built of it."""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, current_stream, lib, ptr

MAX_THRESHOLDS = 8      # D3R_CLOUD_MAX_THRESHOLDS
LADDER_STEP = 4.0
MAX_K = 32              # D3R_CLOUD_MAX_K
# the ladder of `k_nearest`: a rung walks about 27 cells of side r, on a surface sampled at spacing v about 9 r^2 / v^2 points, and resolves
# a query once k points lie within r, about r >= v sqrt(k / pi). A step of 4 from r_0 = 2 v jumps from 36 to 576 points for the queries
# the first rung leaves open (most of them at k = 16, which needs 2.3 v); a step of 2 looks at 144 (tools/cloud_normals_speed.py).
KNN_LADDER_STEP = 2.0
KNN_CELL_FACTOR = 1.0   # cell = factor r of a rung of `k_nearest`; exactness does not depend on it (tools/cloud_normals_speed.py measures 1 and 1/2)


def _radius_f32(x, what):
    """x as np.float32; ValueError unless it is positive and its fp32 square is a normal number (about 1.1e-19 <= x <= 1.8e19): with a
    subnormal or infinite r r the comparison d2 <= r r no longer bounds the coordinates, and the grid's argument needs that"""
    with np.errstate(over='ignore', under='ignore'):
        v = np.float32(x)
        v2 = v * v
    if not (v > 0 and np.isfinite(v2) and v2 >= np.finfo(np.float32).tiny):
        raise ValueError(f'{what} = {x!r} must be a positive float32 whose square is a normal float32')
    return v


def _voxel_of(cloud):
    """the voxel size of a cloud if it has a usable one (a FusedCloud's, finite and positive), else None"""
    voxel = getattr(cloud, 'voxel_size', None)
    return voxel if voxel is not None and math.isfinite(voxel) and voxel > 0 else None


def default_r0(ref, max_dist):
    """the first radius of the ladder: twice the reference cloud's voxel size when it is a FusedCloud with one, else max_dist / 16"""
    voxel = _voxel_of(ref)
    return 2.0 * voxel if voxel is not None else float(max_dist) / 16


def default_knn_r0(ref, k, max_dist):
    """the first radius of the ladder of `k_nearest`: for a FusedCloud with a voxel size v, v max(2, sqrt(k)) -- a surface sampled at
    spacing v holds about pi r^2 / v^2 points within r, so r = v sqrt(k) expects pi k of them (measured on the 12.6 M-point cloud of
    tools/cloud_normals_speed.py at k = 16: 0.4 % of the rows are full at 2 v, 86 % at 4 v); else max_dist / 16"""
    voxel = _voxel_of(ref)
    return voxel * max(2.0, math.sqrt(k)) if voxel is not None else float(max_dist) / 16


def _device_of(*clouds):
    for c in clouds:
        c = getattr(c, 'positions', c)
        if isinstance(c, torch.Tensor) and c.is_cuda:
            return c.device
    return torch.device('cuda')


def _points(cloud, device, what):
    """(N, 3) float32 contiguous on the device, from an array, a tensor or a FusedCloud"""
    p = getattr(cloud, 'positions', cloud)
    t = p if isinstance(p, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.float32)))
    if t.ndim != 2 or t.shape[1] != 3:
        raise ValueError(f'{what}: expected (N, 3) points, got {tuple(t.shape)}')
    if len(t) >= 2 ** 31:
        raise ValueError(f'{what}: {len(t)} points do not fit 31-bit indices')
    return t.to(device=device, dtype=torch.float32).contiguous()


def ladder_radii(r0, max_dist, step=LADDER_STEP):
    """r_k = min(r_0 step^k, max_dist) as float32, step = 4 unless given; the last is exactly max_dist"""
    r0, max_dist = _radius_f32(r0, 'r0'), _radius_f32(max_dist, 'max_dist')
    out, k = [], 0
    while True:
        r = np.float32(min(float(r0) * step ** k, float(max_dist)))
        if not r < max_dist:
            return out + [max_dist]
        out.append(r)
        k += 1


def grid_cell(lo, hi, r):
    """(cell, bits): cell = r, doubled until every axis of the extent fits 21 bits (viz.fuse_key_bits)"""
    from .viz import fuse_key_bits
    cell = np.float32(r)
    while True:
        try:
            return cell, fuse_key_bits(lo, hi, cell)
        except ValueError:
            if not np.isfinite(cell * np.float32(2)):
                raise
            cell = cell * np.float32(2)


def _bounds(pts, device):
    """(lo, hi, n_valid) of the finite points: d3r_fuse_bounds on the cloud as one view of 1 x n. One host synchronisation."""
    n = len(pts)
    ones = torch.ones((n,), dtype=torch.uint8, device=device)
    h, w = torch.ones((1,), dtype=torch.int32, device=device), torch.full((1,), n, dtype=torch.int32, device=device)
    small = torch.empty((4,), dtype=torch.int64, device=device)
    work = _lib.workspace(max(1, lib.d3r_fuse_bounds_workspace_bytes(1, n)), device)
    check(lib.d3r_fuse_bounds(1, ptr(pts), ptr(ones), None, ptr(h), ptr(w), n, ptr(small.view(torch.float32)), ptr(small[3:]), ptr(work),
                              current_stream()), 'fuse_bounds')
    host = small.cpu()
    b = host[:3].view(torch.float32).numpy()
    return b[:3].copy(), b[3:].copy(), int(host[3])


class _ReferenceGrids:
    """The radius ladder over a reference cloud R that does not move, and the only caller of d3r_cloud_grid_build / d3r_cloud_nearest /
    d3r_cloud_knn: rung j searches at radii[j] on a grid of cell cell_factor radii[j], from the second on only for the queries still open.
    k: None for the nearest neighbour (d2 / idx (N,)), else the k nearest (N, k), with exclude_self; evals as `nearest_in_cloud`'s.
    rebuild=False: a workspace per rung, its grid built once here (`register_clouds`: many searches on the same grids). rebuild=True: ONE
    workspace, every rung's grid built in it before its search (one search; the same bytes, tests compare the two). `cluster_points` takes
    a single rung (radii = [eps], rebuild=False) and hands that grid to d3r_cloud_cluster: it never searches."""

    def __init__(self, R, lo, hi, radii, n_query, rebuild=False, k=None, exclude_self=False, cell_factor=1.0, evals=None):
        self.R, self.rebuild, self.k, self.exclude_self, self.evals = R, rebuild, k, bool(exclude_self), evals
        self.lo_c = (C.c_float * 3)(*lo.tolist())
        size = int(lib.d3r_cloud_grid_workspace_bytes(len(R), n_query))
        if size == 0:
            raise ValueError(f'clouds of {n_query} and {len(R)} points are too large')
        work = _lib.workspace(size, R.device) if rebuild else None
        self.rungs = []
        for r in radii:
            cell, bits = grid_cell(lo, hi, _radius_f32(float(r) * cell_factor, 'cell'))
            rung = (float(r), float(cell), (C.c_int * 3)(*bits), work if rebuild else torch.empty(size, dtype=torch.uint8, device=R.device))
            self.rungs.append(rung)
            if not rebuild:
                self._build(rung)

    def _build(self, rung):
        r, cell, bits_c, work = rung
        check(lib.d3r_cloud_grid_build(len(self.R), ptr(self.R), self.lo_c, cell, bits_c, ptr(work), current_stream()), 'cloud_grid_build')

    def search(self, Q, d2, idx):
        """the ladder for the queries Q (at most n_query) into d2 / idx"""
        for j, rung in enumerate(self.rungs):
            if self.rebuild:
                self._build(rung)
            r, cell, bits_c, work = rung
            out = (ptr(d2), ptr(idx), ptr(self.evals), ptr(work), current_stream())
            if self.k is None:
                check(lib.d3r_cloud_nearest(len(self.R), len(Q), ptr(Q), r, self.lo_c, cell, bits_c, int(j > 0), *out), 'cloud_nearest')
            else:
                check(lib.d3r_cloud_knn(len(self.R), len(Q), ptr(Q), self.k, r, self.lo_c, cell, bits_c, int(self.exclude_self), int(j > 0), *out),
                      'cloud_knn')


def _single_grid(P, cell):
    """(grids, used_cell, bits_c, work): ONE grid of the device cloud P, built here at `cell` (`grid_cell`); None without a finite point. One host sync."""
    lo, hi, n_valid = _bounds(P, P.device)
    if n_valid == 0:
        return None
    grids = _ReferenceGrids(P, lo, hi, [cell], 1)
    return (grids,) + grids.rungs[0][1:]


def _ladder_search(Q, R, radii, k, to_host, **how):
    """(d2, idx) of one ladder of the device clouds Q in R: what `nearest_in_cloud` (k None) and `k_nearest` return; `how` as _ReferenceGrids"""
    nq, device = len(Q), Q.device
    shape = (nq,) if k is None else (nq, k)
    d2 = torch.full(shape, float('inf'), dtype=torch.float32, device=device)
    idx = torch.full(shape, -1, dtype=torch.int32, device=device)
    if nq > 0 and len(R) > 0:
        with torch.cuda.device(device):
            lo, hi, n_valid = _bounds(R, device)
            if n_valid > 0:
                _ReferenceGrids(R, lo, hi, radii, nq, rebuild=True, k=k, **how).search(Q, d2, idx)
    if to_host:
        return d2.cpu().numpy(), idx.cpu().numpy()
    return d2, idx


@torch.no_grad()
def nearest_in_cloud(query, ref, max_dist, r0=None, to_host=True, evals=None):
    """(d2, idx) of every query point in `ref` within max_dist, as defined at the top: d2 (N,) float32 squared distances (+inf where none),
    idx (N,) int32 rows of `ref` (-1 where none). query, ref: (N, 3) arrays, tensors or FusedClouds. r0: the first radius of the ladder;
    default twice ref.voxel_size for a FusedCloud, else max_dist / 16. One host synchronisation (the reference cloud's bounds). evals
    (optional): an int32 device tensor (N,) that accumulates the distance evaluations per query (tools/cloud_metrics_speed.py)."""
    max_dist = _radius_f32(max_dist, 'max_dist')
    _lib.require_device()
    device = _device_of(query, ref)
    if r0 is None:
        r0 = default_r0(ref, max_dist)
    radii = ladder_radii(min(float(_radius_f32(r0, 'r0')), float(max_dist)), max_dist)
    Q, R = _points(query, device, 'query'), _points(ref, device, 'ref')
    return _ladder_search(Q, R, radii, None, to_host, evals=evals)


@torch.no_grad()
def k_nearest(query, ref, k, max_dist, exclude_self=False, r0=None, to_host=True, evals=None, step=KNN_LADDER_STEP, cell_factor=KNN_CELL_FACTOR):
    """(d2, idx) of the k nearest neighbours of every query point in `ref` within max_dist: d2 (N, k) float32, idx (N, k) int32. DEFINED
    without a grid (include/dust3r_hip.h, d3r_cloud_knn): the candidates of a query with three finite coordinates are the finite reference
    points with fp32 d2 <= max_dist^2; exclude_self drops the candidate whose INDEX is the query's (query is ref, or a cloud of equal length:
    a duplicate at another index stays); the row holds the k smallest (d2, index) pairs in ascending lexicographic order, padded with
    (+inf, -1). Bit for bit what an fp32 brute force with np.lexsort gives. 1 <= k <= 32. The search is the radius ladder of
    `nearest_in_cloud` with r_j = min(r_0 step^j, max_dist): a query is resolved once its LAST column is found -- every point within r_j was
    looked at, so k candidates within r_j are the k smallest at any larger radius -- and each rung overwrites the rows still open. r0: the
    first radius, default `default_knn_r0`; evals as for `nearest_in_cloud`; cell_factor: the cells of a rung are cell_factor r_j wide (speed
    only). One host synchronisation (the reference cloud's bounds)."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'k_nearest: k = {k} outside [1, {MAX_K}]')
    max_dist = _radius_f32(max_dist, 'max_dist')
    _lib.require_device()
    device = _device_of(query, ref)
    if r0 is None:
        r0 = default_knn_r0(ref, k, max_dist)
    radii = ladder_radii(min(float(_radius_f32(r0, 'r0')), float(max_dist)), max_dist, step=step)
    Q = _points(query, device, 'query')
    R = Q if query is ref else _points(ref, device, 'ref')
    if exclude_self and len(Q) != len(R):
        raise ValueError(f'k_nearest: exclude_self needs query is ref, or clouds of equal length; got {len(Q)} and {len(R)} points')
    return _ladder_search(Q, R, radii, k, to_host, exclude_self=exclude_self, cell_factor=cell_factor, evals=evals)


@torch.no_grad()
def knn_mean_distances(d2, idx):
    """Of the rows of `k_nearest` (device tensors (N, k)): mean (N,) float32 = the mean distance to the k neighbours (fp64 sum of IEEE square
    roots in column order, one rounding), NaN where fewer than k were found; count (1,) int64 = the full rows; sums (2,) float64 = the sum
    of their means and of the means' squares. d3r_cloud_knn_distances; device tensors, no synchronisation."""
    _lib.require_device()
    device = d2.device
    n, k = d2.shape
    mean = torch.full((n,), float('nan'), dtype=torch.float32, device=device)
    count = torch.zeros((1,), dtype=torch.int64, device=device)
    sums = torch.zeros((2,), dtype=torch.float64, device=device)
    if n > 0:
        with torch.cuda.device(device):
            work = _lib.workspace(lib.d3r_cloud_knn_distances_workspace_bytes(n), device)
            check(lib.d3r_cloud_knn_distances(n, k, ptr(d2.contiguous()), ptr(idx.contiguous()), ptr(mean), ptr(count), ptr(sums), ptr(work),
                                              current_stream()), 'cloud_knn_distances')
    return mean, count, sums


def outlier_threshold(count, sum_mean, sum_mean2, std_ratio):
    """mean + std_ratio std of `count` mean neighbour distances from their sum and their sum of squares, host fp64. The std is the sample's
    (count - 1 in the denominator, as Open3D's remove_statistical_outlier; a variance that rounds below zero counts as zero; 0 for fewer
    than two values). NaN when count is 0: no point is kept then."""
    count, s1, s2 = int(count), float(sum_mean), float(sum_mean2)
    if count <= 0:
        return float('nan')
    mean = s1 / count
    var = max(s2 - count * mean * mean, 0.0) / (count - 1) if count > 1 else 0.0
    return mean + float(std_ratio) * math.sqrt(var)


@torch.no_grad()
def cloud_normals(points, ref, idx, min_neighbors=3):
    """(normals (N, 3) float32, curvature (N,) float32) of `points` from the neighbour rows idx (N, k) into `ref`, on the device: per point
    the fp64 scatter matrix of the point and its found neighbours, the unit eigenvector of its smallest eigenvalue l0 (the first component
    of largest magnitude positive) and l0 / (l0 + l1 + l2); the zero normal and NaN with fewer than min_neighbors. d3r_cloud_normals."""
    _lib.require_device()
    device = idx.device
    P = _points(points, device, 'points')
    R = P if points is ref else _points(ref, device, 'ref')
    n, k = idx.shape
    if len(P) != n:
        raise ValueError(f'cloud_normals: {len(P)} points, {n} neighbour rows')
    normals = torch.zeros((n, 3), dtype=torch.float32, device=device)
    curvature = torch.full((n,), float('nan'), dtype=torch.float32, device=device)
    if n > 0 and len(R) > 0:
        with torch.cuda.device(device):
            check(lib.d3r_cloud_normals(n, ptr(P), len(R), ptr(R), k, ptr(idx.contiguous()), int(min_neighbors), ptr(normals), ptr(curvature),
                                        current_stream()), 'cloud_normals')
    return normals, curvature


@torch.no_grad()
def orient_normals(points, normals, depth, conf, intrinsics, cam2world, heights, widths, tol=0.05):
    """`normals` (N, 3) float32 on the device, oriented IN PLACE towards the cameras that see each point; returns n_seen (N,) int32, the
    views in which the point is visible. depth, conf: a scene's padded (n, row) stacks (utils/padded.py), intrinsics (n, 3, 3), cam2world
    (n, 4, 4), heights / widths the int32 shape tables. A view sees a point when it projects in front of the camera onto a pixel whose depth
    agrees within tol (relative); the vote is the confidence-weighted sum of the cosines to the seeing cameras, over all cameras with weight
    1 when none sees it. d3r_cloud_orient_normals."""
    from .utils.geometry import inv
    _lib.require_device()
    device = normals.device
    P = _points(points, device, 'points')
    n, n_views = len(P), len(depth)
    if normals.shape != (n, 3) or normals.dtype != torch.float32 or not normals.is_contiguous():
        raise ValueError(f'orient_normals: normals must be a contiguous float32 ({n}, 3) tensor')
    n_seen = torch.zeros((n,), dtype=torch.int32, device=device)
    if n > 0:
        f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()      # noqa: E731
        depth, conf, cam2world = f32(depth), f32(conf), f32(cam2world)
        if depth.shape != conf.shape or depth.ndim != 2:
            raise ValueError(f'orient_normals: depth {tuple(depth.shape)} and conf {tuple(conf.shape)} must be the same (n, row) stacks')
        centers = cam2world[:, :3, 3].contiguous()
        with torch.cuda.device(device):
            check(lib.d3r_cloud_orient_normals(n, ptr(P), ptr(normals), ptr(n_seen), n_views, ptr(depth), ptr(conf), ptr(f32(intrinsics)),
                                               ptr(f32(inv(cam2world))), ptr(centers), ptr(heights), ptr(widths), depth.shape[1], float(tol),
                                               current_stream()), 'cloud_orient_normals')
    return n_seen


# ---- density clustering ------------------------------------------------------------------------------------------------
Clusters = collections.namedtuple('Clusters', 'labels sizes n_neighbors core')
Clusters.__doc__ = """The result of `cluster_points`: labels (N,) int32, the cluster of every point, -1 for noise; sizes (C,) int32, the members of
cluster 0 .. C - 1, never increasing; n_neighbors (N,) int32, the points within eps, the point itself included; core (N,) bool."""


def _min_points(min_points):
    if isinstance(min_points, bool) or not isinstance(min_points, (int, np.integer)) or min_points < 1 or min_points >= 2 ** 31:
        raise ValueError(f'min_points = {min_points!r} must be an int >= 1')
    return int(min_points)


@torch.no_grad()
def cluster_points(points, eps, min_points=10, to_host=True, evals=None, stage_events=None):
    """`Clusters` of the (N, 3) points (an array, a tensor or a FusedCloud): DBSCAN on the GPU (csrc/cloud_cluster.hip, d3r_cloud_cluster),
    DEFINED without a grid (include/dust3r_hip.h). A point is valid when its coordinates are finite. The neighbours of a valid point are
    the valid points with fp32 d2 <= eps^2 (fp32), THE POINT ITSELF INCLUDED: scikit-learn's convention for min_samples (Open3D's
    cluster_dbscan counts the same way). A point with at least min_points neighbours is core; the clusters are the connected components
    of the core points under d2 <= eps^2, each rooted at its lowest index. A valid non-core point with a core neighbour is a border point
    and takes the cluster of the core neighbour with the smallest (d2, index) pair: unlike textbook DBSCAN, where a border point between
    two clusters goes to whichever reaches it first, the assignment does not depend on any visiting order. Everything else is noise, label
    -1. Clusters are numbered by decreasing size, ties by ascending root. Exactly what an fp32 brute force over all pairs gives; the same
    bytes on every run. Two host synchronisations: the cloud's bounds (for the grid of cell eps), then the number of clusters.
    to_host=False: device tensors. evals: an int32 device tensor (N,) that accumulates the distance evaluations of the counting walk;
    stage_events: four torch.cuda.Event (or None), each recorded once before so that its handle exists, recorded again after the count,
    the components, the border walk and the numbering (tools/cloud_cluster_speed.py)."""
    eps = _radius_f32(eps, 'eps')
    min_points = _min_points(min_points)
    _lib.require_device()
    device = _device_of(points)
    P = _points(points, device, 'points')
    n = len(P)
    labels = torch.full((n,), -1, dtype=torch.int32, device=device)
    n_neighbors = torch.zeros((n,), dtype=torch.int32, device=device)
    core = torch.zeros((n,), dtype=torch.uint8, device=device)
    sizes = torch.zeros((0,), dtype=torch.int32, device=device)
    if n > 0:
        with torch.cuda.device(device):
            single = _single_grid(P, eps)
            if single is not None:
                grids, cell, bits_c, grid = single
                own_bytes = int(lib.d3r_cloud_cluster_workspace_bytes(n))
                if own_bytes == 0:
                    raise ValueError(f'a cloud of {n} points is too large')
                work = _lib.workspace(own_bytes, device)
                all_sizes = torch.empty((n,), dtype=torch.int32, device=device)
                n_clusters = torch.zeros((1,), dtype=torch.int32, device=device)
                events = None
                if stage_events is not None:
                    events = (C.c_void_p * 4)(*[None if e is None else e.cuda_event for e in stage_events])
                check(lib.d3r_cloud_cluster(n, float(eps), min_points, grids.lo_c, cell, bits_c, ptr(labels), ptr(all_sizes), ptr(n_clusters),
                                            ptr(n_neighbors), ptr(core), ptr(evals), events, ptr(grid), ptr(work), current_stream()), 'cloud_cluster')
                sizes = all_sizes[:int(n_clusters.cpu())].clone()            # the one read-back of the clustering
    out = Clusters(labels, sizes, n_neighbors, core.bool())
    return Clusters(*(t.cpu().numpy() for t in out)) if to_host else out


@torch.no_grad()
def distance_stats(points, d2, idx, thresholds):
    """The sums and counts of one direction, on the device: counts (2 + 8,) int64 = (n_valid, n_found, count_j ...), sums (2,) float64 =
    (sum of distances, sum of squared distances) over the found points, median_d2 (1,) float64 = the lower median of d2 over the found
    points (NaN when none). d3r_cloud_distance_stats and d3r_masked_median; no synchronisation."""
    if len(thresholds) > MAX_THRESHOLDS:
        raise ValueError(f'at most {MAX_THRESHOLDS} thresholds, got {len(thresholds)}')
    tau = [float(np.float32(t)) for t in thresholds]
    if not all(math.isfinite(t) and t >= 0 for t in tau):
        raise ValueError(f'thresholds must be finite and >= 0: {list(thresholds)!r}')
    _lib.require_device()
    device = d2.device
    n = len(d2)
    counts = torch.zeros((2 + MAX_THRESHOLDS,), dtype=torch.int64, device=device)
    sums = torch.zeros((2,), dtype=torch.float64, device=device)
    median = torch.full((1,), float('nan'), dtype=torch.float64, device=device)
    if n > 0:
        with torch.cuda.device(device):
            work = _lib.workspace(lib.d3r_cloud_distance_stats_workspace_bytes(n), device)
            check(lib.d3r_cloud_distance_stats(n, ptr(points), ptr(d2), ptr(idx), len(tau), (C.c_float * max(len(tau), 1))(*tau), ptr(counts), ptr(sums),
                                               ptr(work), current_stream()), 'cloud_distance_stats')
            found = (idx >= 0).to(torch.uint8)
            work = _lib.workspace(lib.d3r_pair_criterion_workspace_bytes(1, n), device)
            check(lib.d3r_masked_median(1, n, ptr(d2), None, ptr(found), None, ptr(median), ptr(work), current_stream()), 'masked_median')
    return counts, sums, median


def compose_metrics(pred, gt, thresholds):
    """The dict of `cloud_metrics` from the two directions' numbers; pred, gt: dicts with n_valid, n_found, sum_d, sum_d2, median_d2 and
    counts (one per threshold). Host arithmetic in fp64. The DTU convention: the means run over the FOUND points (pairs beyond max_dist are
    outliers, not clamped), NaN when none is found; precision / recall are over the VALID points, NaN when there is none."""
    def mean(s):
        return s['sum_d'] / s['n_found'] if s['n_found'] > 0 else float('nan')

    def median(s):
        return math.sqrt(s['median_d2']) if s['n_found'] > 0 else float('nan')

    def ratio(a, b):
        return a / b if b > 0 else float('nan')
    acc, comp = mean(pred), mean(gt)
    precision = [ratio(c, pred['n_valid']) for c in pred['counts']]
    recall = [ratio(c, gt['n_valid']) for c in gt['counts']]
    fscore = [0.0 if p + r == 0 else 2 * p * r / (p + r) for p, r in zip(precision, recall)]
    out = dict(accuracy=acc, accuracy_median=median(pred), completeness=comp, completeness_median=median(gt), overall=(acc + comp) / 2,
               thresholds=[float(t) for t in thresholds], precision=precision, recall=recall, fscore=fscore,
               outliers_pred=1 - ratio(pred['n_found'], pred['n_valid']), outliers_gt=1 - ratio(gt['n_found'], gt['n_valid']))
    for side, s in (('pred', pred), ('gt', gt)):
        out.update({f'n_valid_{side}': int(s['n_valid']), f'n_found_{side}': int(s['n_found']), f'sum_d_{side}': float(s['sum_d']),
                    f'sum_d2_{side}': float(s['sum_d2']), f'median_d2_{side}': float(s['median_d2']), f'counts_{side}': [int(c) for c in s['counts']]})
    return out


def _side(counts, sums, median, n_tau):
    counts, sums, median = counts.tolist(), sums.tolist(), median.tolist()
    return dict(n_valid=counts[0], n_found=counts[1], counts=counts[2:2 + n_tau], sum_d=sums[0], sum_d2=sums[1], median_d2=median[0])


@torch.no_grad()
def cloud_metrics(pred, gt, max_dist, thresholds, to_host=True, r0=None, details=None):
    """The metrics of a predicted cloud against a ground-truth cloud, distances truncated at max_dist (see `compose_metrics`):
    accuracy / accuracy_median (pred -> gt), completeness / completeness_median (gt -> pred), overall, precision / recall / fscore per
    threshold, outliers_pred / outliers_gt, and the raw counts and sums. pred, gt: (N, 3) arrays, tensors or FusedClouds. to_host=False:
    the raw device tensors (pred=(counts, sums, median_d2), gt=...) without a synchronisation beyond the two bounds read-backs; compose
    them with `compose_metrics` later. details: a dict that receives d2 / idx of both directions (device tensors)."""
    thresholds = list(thresholds)
    _lib.require_device()
    device = _device_of(pred, gt)
    P, G = _points(pred, device, 'pred'), _points(gt, device, 'gt')
    d2p, ip = nearest_in_cloud(P, G, max_dist, r0=default_r0(gt, max_dist) if r0 is None else r0, to_host=False)
    d2g, ig = nearest_in_cloud(G, P, max_dist, r0=default_r0(pred, max_dist) if r0 is None else r0, to_host=False)
    sp, sg = distance_stats(P, d2p, ip, thresholds), distance_stats(G, d2g, ig, thresholds)
    if details is not None:
        details.update(d2_pred=d2p, idx_pred=ip, d2_gt=d2g, idx_gt=ig)
    if not to_host:
        return dict(pred=sp, gt=sg, thresholds=thresholds)
    packed = torch.cat([t.double() for t in sp + sg]).cpu()            # one read-back (int64 counts are exact in fp64 below 2^53)
    k = 2 + MAX_THRESHOLDS
    cut = lambda o: (packed[o:o + k].long(), packed[o + k:o + k + 2], packed[o + k + 2:o + k + 3])      # noqa: E731
    return compose_metrics(_side(*cut(0), len(thresholds)), _side(*cut(k + 3), len(thresholds)), thresholds)


# ---- registration: Sim(3) ICP ------------------------------------------------------------------------------------------
ICP_POINT_SUMS, ICP_PLANE_SUMS = 18, 36         # the lengths of sums_out of d3r_cloud_icp_sums
ICP_SINGULAR = 1e-12                            # a system whose smallest eigenvalue (singular value) is below this times its largest is singular
METRICS = {'point': 0, 'plane': 1}

Registration = collections.namedtuple('Registration', 'similarity scale rmse n_pairs n_valid iterations converged reason history')
Registration.__doc__ = """The result of `register_clouds`: similarity (4, 4) float64 [s R | t] that takes src onto dst, its scale, rmse and n_pairs
of the last measured iteration (the residual of the metric: distances for 'point', plane distances for 'plane'), n_valid = the finite source
points, iterations (all stages), converged (the LAST stage met the tolerance), reason (why it ended), history = [(stage, n_pairs, rmse)]."""


def similarity_parts(S):
    """(M (12,) float32 = [A | t] row-major, R (9,) float32, scale) of a 4x4 similarity [s R | t; 0 0 0 1], what d3r_cloud_transform takes.
    ValueError unless S is finite, its last row (0, 0, 0, 1) and its 3x3 block a positive multiple of a rotation (to 1e-6)."""
    S = np.asarray(S, np.float64)
    if S.shape != (4, 4) or not np.isfinite(S).all() or not np.array_equal(S[3], [0, 0, 0, 1]):
        raise ValueError(f'expected a finite (4, 4) similarity with last row (0, 0, 0, 1), got {S!r}')
    A = S[:3, :3]
    det = np.linalg.det(A)
    if not det > 0:
        raise ValueError(f'the 3 x 3 block of a similarity has a positive determinant, got {det!r}')
    scale = float(np.cbrt(det))
    R = A / scale
    if not np.abs(R @ R.T - np.eye(3)).max() <= 1e-6:
        raise ValueError('the 3 x 3 block is not a multiple of a rotation')
    return np.concatenate([A, S[:3, 3:4]], axis=1).astype(np.float32).reshape(12), R.astype(np.float32).reshape(9), scale


def exp_so3(w):
    """Rodrigues' formula, fp64: the rotation by |w| about w"""
    w = np.asarray(w, np.float64)
    t = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    a, b = (1 - t * t / 6, 0.5 - t * t / 24) if t < 1e-4 else (math.sin(t) / t, (1 - math.cos(t)) / (t * t))
    return np.eye(3) + a * K + b * (K @ K)


def _about_centre(A, v, centre):
    """the 4x4 map p -> c + A (p - c) + v"""
    out = np.eye(4)
    out[:3, :3] = A
    out[:3, 3] = centre + v - A @ centre
    return out


def icp_update_point(sums, centre, with_scale=True):
    """(delta (4, 4) or None, rmse, reason) from the 18 sums of the point metric about `centre`: weighted Umeyama of the 17 moments
    (bootstrap.similarity_from_moments; with_scale=False: its rotation with scale 1), delta = p -> c + s R (p - c - mx) + my.
    None with a reason when fewer than 3 pairs or the source pairs do not span a plane."""
    from .cloud_opt.bootstrap import similarity_from_moments
    m = np.asarray(sums, np.float64)
    n = m[0]
    rmse = math.sqrt(max(m[17], 0.0) / n) if n > 0 else float('nan')
    if n < 3:
        return None, rmse, f'{int(n)} pairs, 3 needed'
    mx, my = m[1:4] / n, m[4:7] / n
    cov = (m[7:16].reshape(3, 3) / n).T - np.outer(my, mx)
    var = m[16] / n - mx @ mx
    sv = np.linalg.svd(cov, compute_uv=False)
    if not (var > 0 and np.isfinite(sv).all() and sv[1] > ICP_SINGULAR * max(sv[0], var)):
        return None, rmse, 'singular system: the pairs do not fix a rotation'
    T = similarity_from_moments(m[:17])
    s = float(np.cbrt(np.linalg.det(T[:3, :3])))
    if not (np.isfinite(T).all() and s > 0):
        return None, rmse, 'singular system: no finite similarity'
    A = T[:3, :3] if with_scale else T[:3, :3] / s
    return _about_centre(A, my - A @ mx, np.asarray(centre, np.float64)), rmse, None


def plane_system(sums, with_scale=True):
    """(H, g, sum e e) of the 36 sums of the plane metric: H the symmetric 7 x 7 matrix of sum J J^T (its 28 upper-triangle entries
    row-major), g = sum J e; without scale their first six rows and columns"""
    m = np.asarray(sums, np.float64)
    k = 7 if with_scale else 6
    H = np.zeros((7, 7))
    H[np.triu_indices(7)] = m[:28]
    H = H + np.triu(H, 1).T
    return H[:k, :k], m[28:28 + k], float(m[35])


def icp_update_plane(sums, n_pairs, centre, with_scale=True):
    """(delta (4, 4) or None, rmse, reason) from the 36 sums of the plane metric about `centre`: the minimiser x = (omega, v, sigma) of
    sum (e + J x)^2, H x = -g (`plane_system`; 6 unknowns without scale), delta = [e^sigma Exp(omega) | c + v - e^sigma Exp(omega) c].
    Solved after a symmetric diagonal scaling; None with a reason when there are fewer pairs than unknowns or the scaled system's smallest
    eigenvalue is below 1e-12 of its largest."""
    H, g, see = plane_system(sums, with_scale)
    k = len(g)
    rmse = math.sqrt(max(see, 0.0) / n_pairs) if n_pairs > 0 else float('nan')
    if n_pairs < k:
        return None, rmse, f'{int(n_pairs)} pairs, {k} needed'
    d = np.sqrt(np.diag(H))
    if not (np.isfinite(H).all() and np.isfinite(g).all() and (d > 0).all()):
        return None, rmse, 'singular system: a zero or non-finite diagonal'
    Hs = H / np.outer(d, d)
    ev = np.linalg.eigvalsh(Hs)
    if not ev[0] > ICP_SINGULAR * ev[-1]:
        return None, rmse, 'singular system: the planes do not fix every unknown'
    x = np.linalg.solve(Hs, -g / d) / d
    A = (math.exp(x[6]) if k == 7 else 1.0) * exp_so3(x[:3])
    return _about_centre(A, x[3:6], np.asarray(centre, np.float64)), rmse, None


def icp_update(metric, sums, n_pairs, centre, with_scale=True):
    """(delta or None, rmse, reason) of one iteration from what d3r_cloud_icp_sums reduced; metric 'point' or 'plane'"""
    if metric == 'point':
        return icp_update_point(sums, centre, with_scale)
    return icp_update_plane(sums, n_pairs, centre, with_scale)


def _normals_of(cloud, device):
    n = getattr(cloud, 'normals', None)
    if n is None:
        return None
    t = n if isinstance(n, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(n, dtype=np.float32)))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _pca_normals(P, k, radius, r0):
    """PCA normals (N, 3) of the device cloud P, which has none: `cloud_normals` over its k nearest within radius, the ladder from r0"""
    _, nbr = k_nearest(P, P, k, radius, exclude_self=True, r0=min(r0, radius), to_host=False)
    return cloud_normals(P, P, nbr)[0]


@torch.no_grad()
def transform_points(points, S, normals=None, out=None, normals_out=None):
    """points (N, 3) moved by the similarity S, and normals rotated by its rotation, on the device (d3r_cloud_transform): fp32, row r =
    ((A_r0 x + A_r1 y) + A_r2 z) + t_r with [A | t] = float32(S). Device tensors; (moved, rotated normals or None): out / normals_out when given."""
    M, R, _ = similarity_parts(S)
    _lib.require_device()
    device = _device_of(points)
    P = _points(points, device, 'points')
    out = torch.empty_like(P) if out is None else out
    N_in = None if normals is None else _points(normals, device, 'normals')
    if N_in is not None and len(N_in) != len(P):
        raise ValueError(f'transform_points: {len(P)} points, {len(N_in)} normals')
    N_out = None if N_in is None else torch.empty_like(N_in) if normals_out is None else normals_out
    if len(P) > 0:
        with torch.cuda.device(device):
            check(lib.d3r_cloud_transform(len(P), ptr(P), (C.c_float * 12)(*M.tolist()), ptr(out), ptr(N_in), (C.c_float * 9)(*R.tolist()), ptr(N_out),
                                          current_stream()), 'cloud_transform')
    return out, N_out


@torch.no_grad()
def icp_sums(moved, ref, d2, idx, metric, gate, centre, ref_normals=None, moved_normals=None, cos_min=None, want_used=False, out=None):
    """d3r_cloud_icp_sums on device tensors: (count (1,) int64, sums (18 or 36,) float64, used (N,) uint8 or None), no synchronisation.
    out: (count, sums, workspace of d3r_cloud_icp_sums_workspace_bytes(N)) to use instead of allocating them."""
    _lib.require_device()
    device = moved.device
    n = len(moved)
    count, sums, work = out or (torch.zeros((1,), dtype=torch.int64, device=device),
                                torch.zeros((ICP_PLANE_SUMS if METRICS[metric] else ICP_POINT_SUMS,), dtype=torch.float64, device=device), None)
    used = torch.zeros((n,), dtype=torch.uint8, device=device) if want_used else None
    if n > 0 and len(ref) > 0:
        with torch.cuda.device(device):
            work = _lib.workspace(lib.d3r_cloud_icp_sums_workspace_bytes(n), device) if work is None else work
            check(lib.d3r_cloud_icp_sums(n, ptr(moved), ptr(moved_normals), len(ref), ptr(ref), ptr(ref_normals), ptr(d2), ptr(idx), METRICS[metric],
                                         float(gate), 0.0 if cos_min is None else float(cos_min), (C.c_float * 3)(*[float(c) for c in centre]),
                                         ptr(count), ptr(sums), ptr(used), ptr(work), current_stream()), 'cloud_icp_sums')
    return count, sums, used


@torch.no_grad()
def register_clouds(src, dst, max_dist, init=None, with_scale=True, metric='plane', max_iters=30, tol=1e-6, cos_min=None, r0=None, centre=None,
                    _rebuild_grids=False, global_kw=None, details=None):
    """Sim(3) ICP of the cloud src onto the cloud dst on the GPU: a `Registration` whose similarity S takes src into dst's frame.
    src, dst: (N, 3) arrays, tensors or FusedClouds. max_dist: the pair gate, a float or a coarse-to-fine sequence of floats, each a stage
    of at most max_iters iterations that starts where the last ended. init: the (4, 4) similarity to start from (identity). with_scale=False
    keeps the scale of init. metric: 'plane' (point to plane; the normals of dst: its own when it is a FusedCloud with normals, else PCA
    normals of k_nearest(k=16) within 8 voxels, or within the largest max_dist for a cloud without a voxel size) or 'point'. cos_min: pairs
    whose normals (src's rotated by S, dst's) have a cosine below it are dropped; needs normals on both clouds. r0: the first radius of the
    nearest-neighbour ladder (default as `nearest_in_cloud`). centre (3,): the point the sums are taken about, default the middle of dst's
    bounds. One iteration: d3r_cloud_transform of src by float32(S), the ladder of d3r_cloud_nearest on grids built once per stage (dst does
    not move), d3r_cloud_icp_sums, ONE read-back of at most 37 numbers, `icp_update` in fp64 on the host, S <- delta S. A stage ends when
    |rmse - rmse_prev| <= tol rmse (the update of that iteration is not applied: rmse and n_pairs are those of the returned S) or at
    max_iters. ValueError when the first iteration has no pair; later, fewer pairs than unknowns or a singular system end the loop with
    converged=False and a reason. init='global': the loop starts from `global_registration(src, dst, with_scale=with_scale, **global_kw)`
    (DESIGN.md, 4.17), so src may be rotated, moved and scaled by anything; ValueError with its reason when it finds no similarity. The
    `Registration` is the same tuple; the `GlobalRegistration` is put into `details` (a dict, optional) under 'global'."""
    if metric not in METRICS:
        raise ValueError(f"register_clouds: metric is 'point' or 'plane', got {metric!r}")
    stages = [max_dist] if np.ndim(max_dist) == 0 else list(max_dist)
    if not stages or int(max_iters) < 1:
        raise ValueError('register_clouds: max_dist is empty or max_iters < 1')
    stages = [_radius_f32(g, 'max_dist') for g in stages]
    if isinstance(init, str):
        if init != 'global':
            raise ValueError(f"register_clouds: init is a (4, 4) similarity, None or 'global', got {init!r}")
        found = global_registration(src, dst, **dict(dict(with_scale=with_scale), **(global_kw or {})))
        if details is not None:
            details['global'] = found
        if found.similarity is None:
            raise ValueError(f'register_clouds: the global registration found no similarity: {found.reason}')
        init = found.similarity
    elif global_kw is not None:
        raise ValueError("register_clouds: global_kw needs init='global'")
    S = np.eye(4) if init is None else np.array(init, np.float64)
    similarity_parts(S)
    _lib.require_device()
    device = _device_of(src, dst)
    P, Q = _points(src, device, 'src'), _points(dst, device, 'dst')
    n = len(P)
    if n == 0 or len(Q) == 0:
        raise ValueError(f'register_clouds: clouds of {n} and {len(Q)} points')
    src_normals = _normals_of(src, device) if cos_min is not None else None
    dst_normals = _normals_of(dst, device) if metric == 'plane' or cos_min is not None else None
    if cos_min is not None and (src_normals is None or dst_normals is None):
        raise ValueError('register_clouds: cos_min needs normals on both clouds (FusedCloud.estimate_normals)')
    history, reason, converged, rmse, n_pairs, iterations = [], None, False, float('nan'), 0, 0
    with torch.cuda.device(device):
        lo, hi, n_ref_valid = _bounds(Q, device)
        if n_ref_valid == 0:
            raise ValueError('register_clouds: dst has no finite point')
        if metric == 'plane' and dst_normals is None:
            voxel = _voxel_of(dst)
            radius = 8.0 * voxel if voxel is not None else float(max(stages))
            dst_normals = _pca_normals(Q, 16, radius, default_knn_r0(dst, 16, radius))
        n_valid = int(torch.isfinite(P).all(dim=1).sum())
        c = (0.5 * (lo.astype(np.float64) + hi.astype(np.float64))).astype(np.float32) if centre is None else np.asarray(centre, np.float32).reshape(3)
        if not np.isfinite(c).all():
            raise ValueError(f'register_clouds: centre {c!r} is not finite')
        c64 = c.astype(np.float64)
        moved, moved_normals = torch.empty_like(P), None if src_normals is None else torch.empty_like(src_normals)
        d2 = torch.empty((n,), dtype=torch.float32, device=device)
        idx = torch.empty((n,), dtype=torch.int32, device=device)
        count = torch.zeros((1,), dtype=torch.int64, device=device)
        sums = torch.zeros((ICP_PLANE_SUMS if METRICS[metric] else ICP_POINT_SUMS,), dtype=torch.float64, device=device)
        work = _lib.workspace(lib.d3r_cloud_icp_sums_workspace_bytes(n), device)
        for stage, gate in enumerate(stages):
            first = default_r0(dst, gate) if r0 is None else r0
            grids = _ReferenceGrids(Q, lo, hi, ladder_radii(min(float(_radius_f32(first, 'r0')), float(gate)), gate), n, rebuild=_rebuild_grids)
            prev, converged = None, False
            for it in range(int(max_iters)):
                transform_points(P, S, src_normals, out=moved, normals_out=moved_normals)
                grids.search(moved, d2, idx)
                icp_sums(moved, Q, d2, idx, metric, gate, c, dst_normals, moved_normals, cos_min, out=(count, sums, work))
                host = torch.cat([count.double(), sums]).cpu().numpy()          # the iteration's one read-back (the count is exact in fp64)
                pairs = int(host[0])
                if pairs == 0 and not history:
                    raise ValueError(f'register_clouds: no source point has a neighbour within {float(gate)!r} at the initial similarity')
                delta, now, why = icp_update(metric, host[1:], pairs, c64, with_scale)
                iterations += 1
                n_pairs, rmse = pairs, now
                history.append((stage, pairs, now))
                if delta is None:
                    reason = why
                    break
                if prev is not None and abs(now - prev) <= tol * now:
                    converged, reason = True, 'converged'
                    break
                prev = now
                S = delta @ S
            else:
                reason = f'max_iters = {int(max_iters)} reached in stage {stage}'
            if delta is None:
                break
    scale = similarity_parts(S)[2]
    return Registration(S, scale, rmse, n_pairs, n_valid, iterations, converged, reason, history)


# ---- global registration: FPFH features and Sim(3) RANSAC --------------------------------------------------------------
FEATURE_DIM, SPFH_ROW, FEATURE_BINS = 33, 36, 11        # the row of d3r_cloud_fpfh, of d3r_cloud_spfh, the bins of one pair feature
MAX_HYPOTHESES = 1 << 23                                # D3R_SIM3_MAX_HYPOTHESES
FEATURE_CELL = 0.1                                      # the default feature cell, in units of `cloud_size`
FEATURE_KNN_RADIUS = 8.0                                # the descriptor's neighbours lie within this many feature cells
NORMALS_K = 16                                          # the neighbours of the PCA normals of a cloud that has none

GlobalRegistration = collections.namedtuple('GlobalRegistration', 'similarity scale n_features n_matches n_inliers n_valid best_hypothesis mirrored reason')
GlobalRegistration.__doc__ = """The result of `global_registration`: similarity (4, 4) float64 [s R | t] that takes src onto dst (None when none was
found, with the reason), its scale, n_features = (source, destination) feature points, n_matches = the mutual matches RANSAC saw, n_inliers =
the matches within thr of the returned similarity, n_valid = the hypotheses that passed the edge-ratio test, best_hypothesis = the winner's
index, mirrored = whether the run with the source descriptors of reversed normals won, reason (None on success)."""


@torch.no_grad()
def grid_subsample(points, cell, to_host=True):
    """indices (M,) int32: of every occupied cell of the grid of d3r_cloud_grid_build at `cell` (origin = the minimum of the finite points)
    the LOWEST original index among the cell's finite points, in ascending cell-key order (z, then y, then x). d3r_cloud_grid_heads on
    the grid's workspace. ValueError when the extent does not fit 21 bits per axis at that cell. Two host synchronisations (the bounds,
    the count)."""
    cell = _radius_f32(cell, 'cell')
    _lib.require_device()
    device = _device_of(points)
    P = _points(points, device, 'points')
    n = len(P)
    out = torch.empty((0,), dtype=torch.int32, device=device)
    if n > 0:
        with torch.cuda.device(device):
            single = _single_grid(P, cell)
            if single is not None:
                _, used_cell, _, work = single
                if used_cell != float(cell):
                    raise ValueError(f'grid_subsample: cell = {float(cell)!r} is too small for the extent of the cloud')
                heads = torch.empty((n,), dtype=torch.int32, device=device)
                count = torch.zeros((1,), dtype=torch.int32, device=device)
                check(lib.d3r_cloud_grid_heads(n, ptr(heads), ptr(count), ptr(work), current_stream()), 'cloud_grid_heads')
                out = heads[:int(count.cpu())].clone()
    return out.cpu().numpy() if to_host else out


@torch.no_grad()
def cloud_size(points):
    """(size, centroid (3,) float64) of the finite points: size = sqrt(trace of their fp64 covariance), the RMS distance from the centroid.
    (nan, None) for a cloud without a finite point. One host synchronisation."""
    P = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(points, np.float32)))
    V = P[torch.isfinite(P).all(dim=1)].double()
    if len(V) == 0:
        return float('nan'), None
    c = V.mean(dim=0)
    host = torch.cat([((V - c) ** 2).sum(dim=1).mean().reshape(1), c]).cpu().numpy()
    return math.sqrt(float(host[0])), host[1:]


@torch.no_grad()
def feature_cloud(cloud, normals=None, cell=None):
    """(positions (M, 3), normals (M, 3), cell, indices (M,) int32) on the device: the cloud `grid_subsample`d at `cell` (default
    FEATURE_CELL = 0.1 `cloud_size`: relative to the cloud's own size, which makes what follows independent of its unknown scale) and
    the normals at those points. Normals: `normals` when given, else the cloud's own (a FusedCloud with normals), both TAKEN AS CONSISTENTLY
    ORIENTED; else PCA normals of the whole cloud (NORMALS_K = 16 neighbours within 4 cells) turned so that (p - c) . n >= 0 about the
    feature points' centroid c. That orientation suits object-like scans seen from outside; inconsistently oriented normals defeat the
    descriptor."""
    _lib.require_device()
    device = _device_of(cloud)
    P = _points(cloud, device, 'cloud')
    if len(P) == 0:
        raise ValueError('feature_cloud: the cloud is empty')
    if cell is None:
        size, _ = cloud_size(P)
        if not (math.isfinite(size) and size > 0):
            raise ValueError(f'feature_cloud: the cloud has no extent (size {size!r}): give cell')
        cell = FEATURE_CELL * size
    cell = _radius_f32(cell, 'cell')
    own = normals if normals is not None else getattr(cloud, 'normals', None)
    if own is not None:
        own = _points(own, device, 'normals')
        if len(own) != len(P):
            raise ValueError(f'feature_cloud: {len(P)} points, {len(own)} normals')
    idx = grid_subsample(P, cell, to_host=False)
    F = P[idx.long()].contiguous()
    if own is not None:
        return F, own[idx.long()].contiguous(), float(cell), idx
    radius = 4.0 * float(cell)
    N = _pca_normals(P, NORMALS_K, radius, float(cell))[idx.long()]
    c = F.double().mean(dim=0)
    outward = ((F.double() - c) * N.double()).sum(dim=1) >= 0
    return F, torch.where(outward[:, None], N, -N).contiguous(), float(cell), idx


@torch.no_grad()
def spfh_counts(points, normals, idx):
    """counts (N, 36) uint8 of d3r_cloud_spfh (include/dust3r_hip.h has the definition): per point the 3 x 11 histogram of (alpha, phi,
    theta) over its neighbour rows idx (N, k) -- rows of `k_nearest(points, points, k, ..., exclude_self=True)` -- the pairs counted, two
    zero bytes. Device tensors, no synchronisation."""
    _lib.require_device()
    device = idx.device
    P, N = _points(points, device, 'points'), _points(normals, device, 'normals')
    n, k = idx.shape
    if len(P) != n or len(N) != n:
        raise ValueError(f'spfh_counts: {len(P)} points, {len(N)} normals, {n} neighbour rows')
    counts = torch.zeros((n, SPFH_ROW), dtype=torch.uint8, device=device)
    if n > 0:
        with torch.cuda.device(device):
            check(lib.d3r_cloud_spfh(n, ptr(P), ptr(N), k, ptr(idx.contiguous()), ptr(counts), current_stream()), 'cloud_spfh')
    return counts


@torch.no_grad()
def fpfh_features(d2, idx, counts):
    """features (N, 33) float32 of d3r_cloud_fpfh: the point's own histogram plus its neighbours', weighted by normalised 1 / d2, each
    third scaled to sum 100; fp64 in column order. d2, idx (N, k) the rows of `k_nearest`, counts (N, 36) of `spfh_counts`."""
    _lib.require_device()
    device = idx.device
    n, k = idx.shape
    if d2.shape != idx.shape or counts.shape != (n, SPFH_ROW) or counts.dtype != torch.uint8:
        raise ValueError(f'fpfh_features: d2 {tuple(d2.shape)}, idx {tuple(idx.shape)}, counts {tuple(counts.shape)} {counts.dtype}')
    out = torch.zeros((n, FEATURE_DIM), dtype=torch.float32, device=device)
    if n > 0:
        with torch.cuda.device(device):
            check(lib.d3r_cloud_fpfh(n, k, ptr(idx.contiguous()), ptr(d2.contiguous()), ptr(counts.contiguous()), ptr(out), current_stream()), 'cloud_fpfh')
    return out


@torch.no_grad()
def cloud_features(points, normals, cell, k=MAX_K):
    """FPFH features (N, 33) float32 of the feature points: `k_nearest` (k neighbours within FEATURE_KNN_RADIUS = 8 cells, exclude_self),
    `spfh_counts`, `fpfh_features`. Device tensors."""
    radius = FEATURE_KNN_RADIUS * float(cell)
    d2, idx = k_nearest(points, points, k, radius, exclude_self=True, r0=min(float(cell) * max(2.0, math.sqrt(k)), radius), to_host=False)
    return fpfh_features(d2, idx, spfh_counts(points, normals, idx))


def mirror_features(features):
    """the features of the same cloud with every normal negated: a pair's (alpha, phi, theta) becomes (alpha, -phi, -theta), so the phi
    and theta thirds are read in reverse bin order and the alpha third is unchanged. A tensor or an array (N, 33)."""
    b = FEATURE_BINS
    flip = (lambda t: t.flip(1)) if isinstance(features, torch.Tensor) else (lambda t: t[:, ::-1])
    cat = torch.cat if isinstance(features, torch.Tensor) else np.concatenate
    return cat([features[:, :b], flip(features[:, b:2 * b]), flip(features[:, 2 * b:])], 1)


@torch.no_grad()
def feature_nearest(fa, fb):
    """(d2 (Na,) float32, idx (Na,) int32) of every row of fa among the rows of fb, both (N, 33) float32 on the device: the lowest index of
    minimal fp32 squared distance, summed in column order (d3r_feature_nearest: exhaustive and exact); (+inf, -1) for a row with a
    non-finite value and when fb has no finite row."""
    _lib.require_device()
    device = fa.device
    for f in (fa, fb):
        if f.ndim != 2 or f.shape[1] != FEATURE_DIM or f.dtype != torch.float32:
            raise ValueError(f'feature_nearest: expected (N, {FEATURE_DIM}) float32 features, got {tuple(f.shape)} {f.dtype}')
    d2 = torch.full((len(fa),), float('inf'), dtype=torch.float32, device=device)
    idx = torch.full((len(fa),), -1, dtype=torch.int32, device=device)
    if len(fa) > 0 and len(fb) > 0:
        with torch.cuda.device(device):
            check(lib.d3r_feature_nearest(len(fa), ptr(fa.contiguous()), len(fb), ptr(fb.contiguous()), ptr(d2), ptr(idx), current_stream()), 'feature_nearest')
    return d2, idx


@torch.no_grad()
def match_features(fa, fb, mutual=True):
    """(ia, ib) int64 device tensors: row ia[m] of fa matches row ib[m] of fb. `feature_nearest` from fa to fb; mutual=True keeps i <-> j
    only when i is also the nearest of j among fa (a second call the other way), in ascending i."""
    _, ab = feature_nearest(fa, fb)
    ia = torch.nonzero(ab >= 0).reshape(-1)
    ib = ab[ia].long()
    if mutual and len(ia) > 0:
        _, ba = feature_nearest(fb, fa)
        keep = ba[ib].long() == ia
        ia, ib = ia[keep], ib[keep]
    return ia, ib


def _ransac_args(n_hyp, thr, ratio_min):
    if isinstance(n_hyp, bool) or not isinstance(n_hyp, (int, np.integer)) or not 1 <= n_hyp <= MAX_HYPOTHESES:
        raise ValueError(f'n_hyp = {n_hyp!r} must be an int in [1, {MAX_HYPOTHESES}]')
    with np.errstate(over='ignore'):
        t = np.float32(thr)
        ok = t > 0 and np.isfinite(t * t)
    if not ok:
        raise ValueError(f'thr = {thr!r} must be a positive float32 with a finite square')
    if not 0 < float(ratio_min) <= 1:
        raise ValueError(f'ratio_min = {ratio_min!r} must lie in (0, 1]')
    return int(n_hyp), float(t), float(ratio_min)


@torch.no_grad()
def sim3_ransac(p, q, n_hyp, thr, ratio_min=0.9, with_scale=True, seed=0):
    """(best (15,) float64, inliers (n,) uint8) device tensors of d3r_sim3_ransac over the correspondences p[i] <-> q[i] ((n, 3) float32,
    n >= 3): best = (h or -1, inlier count, valid hypotheses, the 12 entries of S = [s R | t] row-major). Hypothesis h: three
    correspondences drawn by (seed, h), rejected unless the three edge-length ratios agree within ratio_min, the similarity of the two
    triangles in fp64; scored in fp32 as `transform_points` then d2 <= thr^2; the largest count wins, then the lowest h. n_hyp is fixed (no
    adaptive stopping); the same seed gives the same bytes. No synchronisation."""
    n_hyp, thr, ratio_min = _ransac_args(n_hyp, thr, ratio_min)
    _lib.require_device()
    device = _device_of(p, q)
    P, Q = _points(p, device, 'p'), _points(q, device, 'q')
    n = len(P)
    if n < 3 or len(Q) != n:
        raise ValueError(f'sim3_ransac: {n} and {len(Q)} points; at least 3 correspondences')
    best = torch.zeros((15,), dtype=torch.float64, device=device)
    inliers = torch.zeros((n,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        work = _lib.workspace(lib.d3r_sim3_ransac_workspace_bytes(n, n_hyp), device)
        check(lib.d3r_sim3_ransac(n, ptr(P), ptr(Q), int(seed) & (2 ** 64 - 1), n_hyp, thr, ratio_min, int(bool(with_scale)), ptr(best), ptr(inliers),
                                  ptr(work), current_stream()), 'sim3_ransac')
    return best, inliers


def similarity_inliers(S, p, q, thr):
    """(n,) bool on the host: the inlier test of d3r_sim3_ransac for the similarity S (4, 4) over p <-> q (n, 3) float32 arrays: p' by the
    fp32 row product of `transform_points`, fp32 d2 <= thr^2, both points finite."""
    M = np.asarray(S, np.float64)[:3, :4].astype(np.float32)
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        moved = np.stack([((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + M[r, 3] for r in range(3)], axis=1)
        d = moved - q
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        t = np.float32(thr)
        return np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1) & (d2 <= t * t)


def refine_on_inliers(S, p, q, thr, with_scale=True, rounds=3):
    """(S, inliers (n,) bool): at most `rounds` rounds of Umeyama over the inlier set of S, host fp64 (`icp_update_point` on the 18 sums of
    the inlier pairs about their destination centroid). A round is kept only when its inlier count does not drop."""
    S = np.array(S, np.float64)
    inl = similarity_inliers(S, p, q, thr)
    p64, q64 = np.asarray(p, np.float64), np.asarray(q, np.float64)
    for _ in range(rounds):
        y = q64[inl]
        c = y.mean(axis=0)
        a = p64[inl] @ S[:3, :3].T + S[:3, 3] - c
        y = y - c
        sums = np.concatenate([[len(a)], a.sum(axis=0), y.sum(axis=0), (a[:, :, None] * y[:, None, :]).sum(axis=0).reshape(9), [(a * a).sum()],
                               [((a - y) ** 2).sum()]])
        delta, _, _ = icp_update_point(sums, c, with_scale)
        if delta is None:
            break
        S_new = delta @ S
        inl_new = similarity_inliers(S_new, p, q, thr)
        if inl_new.sum() < inl.sum():
            break
        same = np.array_equal(inl_new, inl)
        S, inl = S_new, inl_new
        if same:
            break
    return S, inl


@torch.no_grad()
def global_registration(src, dst, src_normals=None, dst_normals=None, cell=None, k=MAX_K, n_hyp=65536, thr=None, ratio_min=0.9, with_scale=True,
                        seed=0, try_mirrored=True, to_host=True):
    """Global (initialisation-free) registration of the cloud src onto the cloud dst on the GPU: a `GlobalRegistration` whose similarity
    takes src into dst's frame from ANY relative rotation, translation and (with_scale) scale -- the coarse similarity `register_clouds`
    needs. src, dst: (N, 3) arrays, tensors or FusedClouds.
    1. `feature_cloud` of both sides: cell = None takes 0.1 of each cloud's own size, a float is the cell of BOTH clouds (then they
       must share a scale), a pair is (source cell, destination cell). Normals: src_normals / dst_normals, else the clouds' own, else oriented PCA normals (see `feature_cloud`:
       that orientation suits object-like scans; inconsistently oriented normals defeat the descriptor).
    2. `cloud_features` on each: k nearest neighbours, SPFH, FPFH.
    3. `match_features`: mutual nearest neighbours in the 33-dimensional feature space, exhaustive.
    4. `sim3_ransac` over the matches, thr defaulting to half the destination's feature cell, n_hyp hypotheses, the given seed.
       try_mirrored: a second match and RANSAC with `mirror_features` of the source -- the descriptors the source would have with every
       normal negated -- covers a cloud whose normals point the other way; the higher inlier count wins, ties go to the unmirrored run.
    5. `refine_on_inliers`: at most three rounds of Umeyama over the inliers, fp64 on the host; the matches are read back once for it.
    Fewer than 3 matches, or no hypothesis with 3 inliers, gives similarity=None with a reason, not an exception. The result is host
    data whatever to_host says (the argument exists for symmetry with the other calls of this module)."""
    n_hyp, _, ratio_min = _ransac_args(n_hyp, 1.0 if thr is None else thr, ratio_min)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f'global_registration: k = {k} outside [1, {MAX_K}]')
    _lib.require_device()
    device = _device_of(src, dst)
    with torch.cuda.device(device):
        cells = (cell, cell) if cell is None or np.ndim(cell) == 0 else tuple(cell)
        Ps, Ns, cell_s, _ = feature_cloud(_as_cloud(src, device), src_normals, cells[0])
        Pd, Nd, cell_d, _ = feature_cloud(_as_cloud(dst, device), dst_normals, cells[1])
        n_features = (len(Ps), len(Pd))
        thr = 0.5 * cell_d if thr is None else thr
        fail = lambda why, n_matches=0, n_valid=0: GlobalRegistration(None, float('nan'), n_features, n_matches, 0, n_valid, -1, False, why)      # noqa: E731
        Fs, Fd = cloud_features(Ps, Ns, cell_s, k), cloud_features(Pd, Nd, cell_d, k)
        runs = []
        for mirrored in ([False, True] if try_mirrored else [False]):
            ia, ib = match_features(mirror_features(Fs) if mirrored else Fs, Fd)
            if len(ia) < 3:
                runs.append((None, None, None, len(ia)))
                continue
            p, q = Ps[ia].contiguous(), Pd[ib].contiguous()
            best, _ = sim3_ransac(p, q, n_hyp, thr, ratio_min, with_scale, seed)
            runs.append((best.cpu().numpy(), p, q, len(ia)))
        counts = [-1 if b is None else (int(b[1]) if b[0] >= 0 else 0) for b, _, _, _ in runs]
        w = int(np.argmax(counts))                                          # the first of equal counts: the unmirrored run
        best, p, q, n_matches = runs[w]
        if best is None:
            return fail(f'{max(r[3] for r in runs)} mutual matches, 3 needed', max(r[3] for r in runs))
        if best[0] < 0:
            return fail(f'no hypothesis of {n_hyp} ({int(best[2])} valid) has 3 inliers within {float(thr)!r}', n_matches, int(best[2]))
        S0 = np.eye(4)
        S0[:3, :4] = best[3:].reshape(3, 4)
        S, inl = refine_on_inliers(S0, p.cpu().numpy(), q.cpu().numpy(), thr, with_scale)        # the one read-back of the matches
    return GlobalRegistration(S, similarity_parts(S)[2], n_features, n_matches, int(inl.sum()), int(best[2]), int(best[0]), bool(w), None)


def _as_cloud(cloud, device):
    """a FusedCloud as it is (its normals and positions are read by name), anything else as device points"""
    return cloud if hasattr(cloud, 'positions') else _points(cloud, device, 'cloud')


# ---- planes: RANSAC on the whole cloud, refit on the moments of the inliers, sequential extraction ------------------------
MAX_HYPOTHESES_PLANE = MAX_HYPOTHESES       # D3R_SIM3_MAX_HYPOTHESES bounds the plane RANSAC too
PLANE_MOMENTS = 9
Plane = collections.namedtuple('Plane', 'model inliers count rms')
Planes = collections.namedtuple('Planes', 'planes plane_sizes plane_labels')


def _plane_args(thr, n_hyp=1, cos_min=None, min_area2=None, min_inliers=3):
    """(thr, n_hyp, cos_min, min_area2, min_inliers) as the device calls take them; ValueError for what d3r_plane_ransac would refuse.
    min_area2 = None: (8 thr)^2 -- twice the area of a right triangle with legs of 8 thr: a sample whose points err by thr then tilts its
    plane by about thr / (8 thr), 7 degrees, at the most, and the refit takes it from there."""
    if isinstance(n_hyp, bool) or not isinstance(n_hyp, (int, np.integer)) or not 1 <= n_hyp <= MAX_HYPOTHESES_PLANE:
        raise ValueError(f'n_hyp = {n_hyp!r} must be an int in [1, {MAX_HYPOTHESES_PLANE}]')
    with np.errstate(over='ignore'):
        t = np.float32(thr)
    if not (t > 0 and np.isfinite(t)):
        raise ValueError(f'thr = {thr!r} must be a positive finite float32')
    cos_min = 0.0 if cos_min is None else float(np.float32(cos_min))
    if math.isnan(cos_min):
        raise ValueError('cos_min is NaN')
    min_area2 = (8.0 * float(t)) ** 2 if min_area2 is None else float(min_area2)
    if not min_area2 > 0:
        raise ValueError(f'min_area2 = {min_area2!r} must be > 0')
    if isinstance(min_inliers, bool) or not isinstance(min_inliers, (int, np.integer)) or not 3 <= min_inliers < 2 ** 31:
        raise ValueError(f'min_inliers = {min_inliers!r} must be an int >= 3')
    return float(t), int(n_hyp), cos_min, min_area2, int(min_inliers)


def _plane_cloud(points, normals, device, what):
    P = _points(points, device, what)
    N = None if normals is None else _points(normals, device, 'normals')
    if N is not None and len(N) != len(P):
        raise ValueError(f'{what}: {len(P)} points, {len(N)} normals')
    return P, N


@torch.no_grad()
def plane_ransac(points, thr, n_hyp=4096, normals=None, cos_min=None, min_area2=None, min_inliers=3, seed=0):
    """(best (7,) float64, inliers (n,) uint8) device tensors of d3r_plane_ransac over the points ((n, 3) float32, n >= 3): best = (h or
    -1, inlier count, valid hypotheses, n_x, n_y, n_z, d). Hypothesis h: three points drawn by (seed, h), the plane through them in fp64,
    rejected unless twice the triangle's area is >= min_area2 (default (8 thr)^2); scored in fp32 as |n . x + d| <= thr and, with normals
    (n, 3), |n . normal| >= cos_min (default 0: then the normals only exclude the points that have none); the largest count wins, then
    the lowest h; -1 unless that count >= min_inliers. n_hyp is fixed (no adaptive stopping); the same seed gives the same bytes. No
    synchronisation."""
    thr, n_hyp, cos_min, min_area2, min_inliers = _plane_args(thr, n_hyp, cos_min, min_area2, min_inliers)
    _lib.require_device()
    device = _device_of(points)
    P, N = _plane_cloud(points, normals, device, 'plane_ransac')
    n = len(P)
    if n < 3:
        raise ValueError(f'plane_ransac: {n} points; at least 3')
    best = torch.zeros((7,), dtype=torch.float64, device=device)
    inliers = torch.zeros((n,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        work = _lib.workspace(lib.d3r_plane_ransac_workspace_bytes(n, n_hyp), device)
        check(lib.d3r_plane_ransac(n, ptr(P), ptr(N), int(seed) & (2 ** 64 - 1), n_hyp, thr, cos_min, min_area2, min_inliers, ptr(best), ptr(inliers),
                                   ptr(work), current_stream()), 'plane_ransac')
    return best, inliers


@torch.no_grad()
def plane_support(points, plane, thr, centre, normals=None, cos_min=None, want_mask=True):
    """d3r_plane_support on device tensors: (count (1,) int64, sums (9,) float64, mask (n,) uint8 or None) of the inliers of `plane`
    (4,), taken as float32: the inlier test of `plane_ransac`, and the fp64 moments of the inliers about `centre` (3,) float32 -- sum a
    and the upper triangle of sum a a^T, a = p - centre. One launch pair, no synchronisation."""
    thr, _, cos_min, _, _ = _plane_args(thr, cos_min=cos_min)
    m = [float(v) for v in np.asarray(plane, np.float64).astype(np.float32).reshape(4)]
    c = [float(v) for v in np.asarray(centre, np.float64).astype(np.float32).reshape(3)]
    if not np.isfinite(m + c).all():
        raise ValueError(f'plane_support: plane {m} and centre {c} must be finite in float32')
    _lib.require_device()
    device = _device_of(points)
    P, N = _plane_cloud(points, normals, device, 'plane_support')
    n = len(P)
    count = torch.zeros((1,), dtype=torch.int64, device=device)
    sums = torch.zeros((PLANE_MOMENTS,), dtype=torch.float64, device=device)
    mask = torch.zeros((n,), dtype=torch.uint8, device=device) if want_mask else None
    if n > 0:
        with torch.cuda.device(device):
            work = _lib.workspace(lib.d3r_plane_support_workspace_bytes(n), device)
            check(lib.d3r_plane_support(n, ptr(P), ptr(N), (C.c_float * 4)(*m), thr, cos_min, (C.c_float * 3)(*c), ptr(mask), ptr(count), ptr(sums),
                                        ptr(work), current_stream()), 'plane_support')
    return count, sums, mask


def moments_covariance(count, sums):
    """(mean of a (3,), covariance (3, 3)) in fp64 of `count` points from their 9 moments about a centre (`plane_support`)"""
    s = np.asarray(sums, np.float64)
    mean = s[:3] / count
    second = np.array([[s[3], s[4], s[5]], [s[4], s[6], s[7]], [s[5], s[7], s[8]]]) / count
    return mean, second - np.outer(mean, mean)


def plane_from_moments(count, sums, centre):
    """The least-squares plane (4,) float64 = (n, d) of `count` points given their 9 moments about `centre` (`plane_support`): through the
    centroid, n the unit eigenvector of the covariance's smallest eigenvalue (np.linalg.eigh), signed so that its component of largest
    magnitude is positive, d = -n . centroid. None for fewer than 3 points or moments that are not finite. Host fp64."""
    if count < 3 or not np.isfinite(np.asarray(sums, np.float64)).all():
        return None
    mean, cov = moments_covariance(count, sums)
    _, vec = np.linalg.eigh(cov)
    n = vec[:, 0] / np.linalg.norm(vec[:, 0])
    if n[int(np.argmax(np.abs(n)))] < 0:
        n = -n
    centroid = np.asarray(centre, np.float64) + mean
    return np.array([n[0], n[1], n[2], -float(n @ centroid)])


def plane_rms(model, count, sums, centre):
    """sqrt(mean e^2), e = n . p + d, over the `count` points whose 9 moments about `centre` are `sums`: from the moments, no pass over
    the points. sum e^2 = n^T (sum a a^T) n + 2 k n . (sum a) + count k^2 with k = n . centre + d."""
    if count <= 0:
        return float('nan')
    s = np.asarray(sums, np.float64)
    n, d = np.asarray(model, np.float64)[:3], float(model[3])
    A = np.array([[s[3], s[4], s[5]], [s[4], s[6], s[7]], [s[5], s[7], s[8]]])
    k = float(n @ np.asarray(centre, np.float64)) + d
    return math.sqrt(max(float(n @ A @ n) + 2.0 * k * float(n @ s[:3]) + count * k * k, 0.0) / count)


def plane_centre(model):
    """(3,) float32: the point of the plane nearest the origin, -d n: the centre the refit's moments are taken about"""
    m = np.asarray(model, np.float64)
    return (-m[3] * m[:3]).astype(np.float32)


def _segment(P, N, thr, n_hyp, cos_min, min_area2, min_inliers, seed, refine_rounds):
    """segment_plane on device tensors: (model, mask uint8 device tensor, count, rms) or None"""
    best, _ = plane_ransac(P, thr, n_hyp, N, cos_min, min_area2, min_inliers, seed)
    best = best.cpu().numpy()
    if best[0] < 0:
        return None
    model = best[3:7].copy()
    centre = plane_centre(model)
    previous = None
    for r in range(refine_rounds + 1):
        count_d, sums_d, mask = plane_support(P, model, thr, centre, N, cos_min)
        packed = torch.cat([count_d.double(), sums_d]).cpu().numpy()      # the round's one read-back: ten numbers
        count, sums = int(packed[0]), packed[1:]
        if r == refine_rounds or count == previous:
            break
        refit = plane_from_moments(count, sums, centre)
        if refit is None or not np.isfinite(refit.astype(np.float32)).all():
            break
        model, previous = refit, count
    return model, mask, count, plane_rms(model, count, sums, centre)


def _plane_normals(cloud, normals, cos_min, device):
    """the normals of the inlier test: those given; else, when cos_min is given, the cloud's own"""
    if normals is not None:
        return normals
    if cos_min is None:
        return None
    own = _normals_of(cloud, device)
    if own is None:
        raise ValueError('cos_min needs normals: give them, or a cloud that has them (estimate_normals)')
    return own


def _rounds(refine_rounds):
    if isinstance(refine_rounds, bool) or not isinstance(refine_rounds, (int, np.integer)) or refine_rounds < 0:
        raise ValueError(f'refine_rounds = {refine_rounds!r} must be an int >= 0')
    return int(refine_rounds)


@torch.no_grad()
def segment_plane(cloud, thr, n_hyp=4096, normals=None, cos_min=None, min_area2=None, min_inliers=3, seed=0, refine_rounds=3, to_host=True):
    """The dominant plane of a cloud ((N, 3) points or a FusedCloud) on the GPU: a `Plane`(model (4,) float64 = (n, d), inliers (N,) bool,
    count, rms), or None when no hypothesis has min_inliers inliers. 1. `plane_ransac`. 2. At most refine_rounds refits: `plane_support`
    of the current model (as float32) gives its mask, count and moments about `plane_centre` of the RANSAC plane in one launch and one
    read-back of ten numbers; `plane_from_moments` of them is the next model. It stops early when the count equals the previous round's.
    The model returned is the last one whose mask was taken: inliers, count and rms (`plane_rms`, from the same moments) are its own.
    normals / cos_min: as `plane_ransac`; with cos_min and no normals the cloud's own are used. The mask comes back on the host unless
    to_host=False."""
    args = _plane_args(thr, n_hyp, cos_min, min_area2, min_inliers)
    refine_rounds = _rounds(refine_rounds)
    _lib.require_device()
    device = _device_of(cloud)
    with torch.cuda.device(device):
        P, N = _plane_cloud(cloud, _plane_normals(cloud, normals, cos_min, device), device, 'segment_plane')
        if len(P) < 3:
            return None
        res = _segment(P, N, args[0], args[1], None if N is None else args[2], args[3], args[4], seed, refine_rounds)
    if res is None:
        return None
    model, mask, count, rms = res
    mask = mask.bool()
    return Plane(model, mask.cpu().numpy() if to_host else mask, count, rms)


def default_plane_min_inliers(n):
    """the support below which `detect_planes` stops: 2 % of the cloud, at least 3 -- a floor or a wall of a scene holds far more, and a
    plane through fewer points is found in any clutter"""
    return max(3, int(math.ceil(0.02 * n)))


@torch.no_grad()
def detect_planes(cloud, thr, max_planes=6, min_inliers=None, n_hyp=4096, normals=None, cos_min=None, min_area2=None, seed=0, refine_rounds=3,
                  to_host=True):
    """The planes of a cloud by sequential extraction on the GPU: `Planes`(planes (P, 4) float64, plane_sizes (P,) int32, plane_labels (N,)
    int32, -1 = no plane), in extraction order. Round r runs `segment_plane` with seed + r on the points no earlier plane took -- they are
    neither sampled nor scored: a boolean compaction on the device keeps the map back to the rows -- and stops at max_planes, when fewer
    than 3 points are left, or at the first round without a plane of min_inliers points (default `default_plane_min_inliers` of the whole
    cloud), before or after the refit. Sizes and labels come back on the host unless to_host=False."""
    if isinstance(max_planes, bool) or not isinstance(max_planes, (int, np.integer)) or max_planes < 0:
        raise ValueError(f'max_planes = {max_planes!r} must be an int >= 0')
    refine_rounds = _rounds(refine_rounds)
    n_all = len(getattr(cloud, 'positions', cloud))
    args = _plane_args(thr, n_hyp, cos_min, min_area2, default_plane_min_inliers(n_all) if min_inliers is None else min_inliers)
    _lib.require_device()
    device = _device_of(cloud)
    with torch.cuda.device(device):
        P, N = _plane_cloud(cloud, _plane_normals(cloud, normals, cos_min, device), device, 'detect_planes')
        labels = torch.full((len(P),), -1, dtype=torch.int32, device=device)
        rows = torch.arange(len(P), device=device)
        planes, sizes = [], []
        for r in range(int(max_planes)):
            if len(P) < 3:
                break
            res = _segment(P, N, args[0], args[1], None if N is None else args[2], args[3], args[4], int(seed) + r, refine_rounds)
            if res is None or res[2] < args[4]:
                break
            model, mask, count, _ = res
            taken = mask.bool()
            labels[rows[taken]] = r
            planes.append(model)
            sizes.append(count)
            rows, P = rows[~taken], P[~taken].contiguous()
            N = None if N is None else N[~taken].contiguous()
    planes = np.array(planes, np.float64).reshape(-1, 4)
    sizes = np.array(sizes, np.int32)
    if to_host:
        return Planes(planes, sizes, labels.cpu().numpy())
    return Planes(planes, torch.from_numpy(sizes).to(device), labels)


def ground_plane(planes, sizes, cam_centres, thr):
    """The ground among detected planes: the plane of largest support (the first of equals) that has EVERY camera centre strictly on one
    side, at more than thr -- cameras stand above a floor, while a wall or a table usually has one behind or below it. Returned (4,)
    float64 with the sign that puts the cameras on its positive side (n . c + d > thr), or None when there is none. Host fp64."""
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    sizes = np.asarray(sizes).reshape(-1)
    C3 = np.asarray(cam_centres, np.float64).reshape(-1, 3)
    if len(planes) != len(sizes):
        raise ValueError(f'ground_plane: {len(planes)} planes, {len(sizes)} sizes')
    if len(C3) == 0 or not thr >= 0:
        raise ValueError('ground_plane: needs camera centres and thr >= 0')
    for k in np.argsort(-sizes.astype(np.int64), kind='stable'):
        e = C3 @ planes[k, :3] + planes[k, 3]
        if (e > thr).all():
            return planes[k].copy()
        if (e < -thr).all():
            return -planes[k]
    return None


def upright_similarity(plane, up=(0.0, 1.0, 0.0)):
    """The (4, 4) rigid motion of least angle that takes the plane's normal to `up` and the plane to height 0 (up . x' = 0 for x on the
    plane): R = the rotation about n x up by the angle between them (about any axis perpendicular to n when n = -up), t = d up. Host fp64."""
    m = np.asarray(plane, np.float64).reshape(4)
    u = np.asarray(up, np.float64).reshape(3)
    ln, lu = np.linalg.norm(m[:3]), np.linalg.norm(u)
    if not (ln > 0 and lu > 0 and np.isfinite(m).all() and np.isfinite(u).all()):
        raise ValueError(f'upright_similarity: plane {m.tolist()} / up {u.tolist()} have no direction')
    n, d, u = m[:3] / ln, m[3] / ln, u / lu
    axis = np.cross(n, u)
    s, c = np.linalg.norm(axis), float(n @ u)
    if s > 1e-12:
        k = axis / s
    else:                                                               # parallel: nothing to do, or half a turn about any perpendicular axis
        k = np.cross(n, np.eye(3)[int(np.argmin(np.abs(n)))])
        k /= np.linalg.norm(k)
        s, c = 0.0, (1.0 if c > 0 else -1.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + s * K + (1.0 - c) * (K @ K)
    T[:3, 3] = d * u
    return T


def transform_planes(planes, S):
    """planes (P, 4) mapped by the similarity S = [s R | t]: n' = R n, d' = s d - n' . t, so that n' . (S x) + d' = s (n . x + d)"""
    planes = np.asarray(planes, np.float64).reshape(-1, 4)
    _, _, scale = similarity_parts(S)
    S = np.asarray(S, np.float64)
    R = S[:3, :3] / scale
    n = planes[:, :3] @ R.T
    return np.concatenate([n, (scale * planes[:, 3] - n @ S[:3, 3])[:, None]], axis=1)
