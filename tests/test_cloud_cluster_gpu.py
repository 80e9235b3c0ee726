"""Density clustering on the GPU: csrc/cloud_cluster.hip (cloud_metrics.cluster_points, FusedCloud.cluster / keep_clusters,
scene.fuse(clusters=...)) against the restatement of tests/test_cloud_cluster_cpu.py. Everything is compared EXACTLY (np.array_equal on
labels, sizes, n_neighbors and core): the definition is an fp32 brute force over all pairs and the kernels evaluate the same fp32 expression
on a subset that holds every point within eps; the components, the border rule and the numbering do not depend on any order.

The large clouds (a 65 537-point chain, a 200 000-point lattice) are too big for the all-pairs restatement. They live on the lattice 2^-6 *
integers with eps = 1.5 units: every coordinate and difference is exact in fp32, every d2 is an integer multiple of 2^-12 (0, 1, 2, 3, ...
units^2) formed without rounding, and eps2 = 2.25 units^2 lies between two attainable values. An fp64 cKDTree.query_pairs +
connected_components oracle (`lattice_oracle`) therefore decides every pair as the fp32 definition does, and the two agree exactly."""
import numpy as np
import pytest
import torch

from test_cloud_cluster_cpu import PARAMS, SCENE, partition_of, restated_dbscan, scene_restated
from test_cloud_metrics_cpu import lattice_case, restated_grid_nearest

pytestmark = pytest.mark.gpu

F32 = np.float32
UNIT = 2.0 ** -6


def _run(P, eps, min_points, **kw):
    from dust3r_amd.cloud_metrics import cluster_points
    return cluster_points(P, eps, min_points=min_points, **kw)


def _same(got, want):
    assert got.labels.dtype == np.int32 and got.sizes.dtype == np.int32 and got.n_neighbors.dtype == np.int32 and got.core.dtype == bool
    assert np.array_equal(got.n_neighbors, want.n_neighbors)
    assert np.array_equal(got.core, want.core)
    assert np.array_equal(got.sizes, want.sizes)
    assert np.array_equal(got.labels, want.labels)


# ---- 1. exactness against the restatement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eps,min_points', PARAMS)
def test_scene_is_clustered_exactly_and_the_same_twice(gpu, eps, min_points):
    want = scene_restated(eps, min_points)
    a = _run(torch.from_numpy(SCENE).to(gpu), eps, min_points)
    b = _run(SCENE, eps, min_points)
    _same(a, want)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    dev = _run(torch.from_numpy(SCENE).to(gpu), eps, min_points, to_host=False)
    assert all(t.is_cuda for t in dev) and dev.core.dtype == torch.bool and np.array_equal(dev.labels.cpu().numpy(), want.labels)


# ---- 2. lattice clouds against the cKDTree oracle -------------------------------------------------------------------------------------------
def lattice_oracle(Q, eps_units, min_points):
    """(labels, sizes, n_neighbors, core) of integer lattice points Q (n, 3) int64, distances in lattice units, by fp64 cKDTree.query_pairs
    and connected_components: exact on the lattice (the module's docstring)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    n = len(Q)
    pairs = cKDTree(Q.astype(np.float64)).query_pairs(float(eps_units), output_type='ndarray')
    i, j = pairs[:, 0], pairs[:, 1]
    n_neighbors = (1 + np.bincount(pairs.ravel(), minlength=n)).astype(np.int32)
    core = n_neighbors >= min_points
    both = core[i] & core[j]
    _, comp = connected_components(coo_matrix((np.ones(both.sum(), np.int8), (i[both], j[both])), shape=(n, n)), directed=False)
    comp_root = np.full(n, n, np.int64)
    np.minimum.at(comp_root, comp[core], np.nonzero(core)[0])
    roots = np.where(core, comp_root[comp], -1)
    # border: over the pairs of one core and one other point, the smallest (d2, core index) per other point
    a = np.concatenate([i[core[j] & ~core[i]], j[core[i] & ~core[j]]])     # the point that is not core
    c = np.concatenate([j[core[j] & ~core[i]], i[core[i] & ~core[j]]])     # its core neighbour
    d2 = ((Q[a] - Q[c]) ** 2).sum(axis=1)
    order = np.lexsort((c, d2, a))
    first = np.ones(len(order), bool)
    first[1:] = a[order][1:] != a[order][:-1]
    roots[a[order][first]] = roots[c[order][first]]
    uniq, sizes = np.unique(roots[roots >= 0], return_counts=True)
    rank = np.empty(len(uniq), np.int64)
    by_size = np.lexsort((uniq, -sizes))
    rank[by_size] = np.arange(len(uniq))
    labels = np.full(n, -1, np.int32)
    labels[roots >= 0] = rank[np.searchsorted(uniq, roots[roots >= 0])]
    return labels, sizes[by_size].astype(np.int32), n_neighbors, core


def test_lattice_oracle_is_the_restatement_on_a_small_lattice():
    """the oracle itself, held against the all-pairs fp32 definition where that still fits"""
    rng = np.random.default_rng(11)
    Q = np.unique(rng.integers(0, 14, (1500, 3)), axis=0)
    Q = Q[rng.permutation(len(Q))].astype(np.int64)
    want = restated_dbscan((Q * UNIT).astype(F32), 1.5 * UNIT, 7)
    labels, sizes, n_neighbors, core = lattice_oracle(Q, 1.5, 7)
    assert 0 < core.sum() < len(Q) and ((labels >= 0) & ~core).any() and (labels < 0).any() and len(sizes) > 1
    assert np.array_equal(labels, want.labels) and np.array_equal(sizes, want.sizes) and np.array_equal(n_neighbors, want.n_neighbors)
    assert np.array_equal(core, want.core)


CHAIN = 65537


def test_a_long_thin_chain_is_one_cluster(gpu):
    """65 537 points in a row, one unit apart, indices permuted: the smallest shape that breaks a capped number of propagation rounds or an
    unflattened forest. Every point has its two neighbours and itself within 1.5 units (the ends one), so with min_points = 2 all are core."""
    rng = np.random.default_rng(21)
    Q = np.zeros((CHAIN, 3), np.int64)
    Q[:, 0] = rng.permutation(CHAIN)
    got = _run((Q * UNIT).astype(F32), 1.5 * UNIT, 2)
    assert got.sizes.tolist() == [CHAIN] and (got.labels == 0).all() and got.core.all()
    ends = (Q[:, 0] == 0) | (Q[:, 0] == CHAIN - 1)
    assert (got.n_neighbors[ends] == 2).all() and (got.n_neighbors[~ends] == 3).all()


def test_two_chains_three_units_apart_stay_two_clusters(gpu):
    rng = np.random.default_rng(22)
    Q = np.zeros((2 * CHAIN, 3), np.int64)
    Q[:CHAIN, 0], Q[CHAIN:, 0], Q[CHAIN:, 1] = np.arange(CHAIN), np.arange(CHAIN), 3
    which = np.arange(2 * CHAIN) >= CHAIN
    perm = rng.permutation(2 * CHAIN)
    Q, which = Q[perm], which[perm]
    got = _run((Q * UNIT).astype(F32), 1.5 * UNIT, 2)
    assert got.sizes.tolist() == [CHAIN, CHAIN] and got.core.all()
    assert len(set(got.labels[which].tolist())) == 1 and len(set(got.labels[~which].tolist())) == 1
    assert got.labels[0] == 0 and got.labels[which][0] != got.labels[~which][0]      # equal sizes: the chain that holds index 0 is cluster 0
    labels, sizes, n_neighbors, core = lattice_oracle(Q, 1.5, 2)
    assert np.array_equal(got.labels, labels) and np.array_equal(got.n_neighbors, n_neighbors)


def test_dense_lattice_cloud_against_the_oracle(gpu):
    """200 000 points: a random 38 % of an 80^3 lattice (about 7 of the 19 sites within 1.5 units are taken, so min_points = 8 leaves core,
    border and noise points side by side) and three solid blobs off to one side. Cells of 1.5 units hold several points each, and the cloud
    spans every workgroup boundary."""
    rng = np.random.default_rng(23)
    side, n_blob = 80, 3 * 12 ** 3
    sites = rng.choice(side ** 3, 200_000 - n_blob, replace=False)
    bulk = np.stack([sites % side, (sites // side) % side, sites // side ** 2], axis=1)
    cube = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
    blobs = [cube + np.array(o) for o in ((100, 0, 0), (100, 30, 0), (100, 30, 30))]
    Q = np.concatenate([bulk] + blobs).astype(np.int64)
    Q = Q[rng.permutation(len(Q))]
    assert len(Q) == 200_000
    got = _run((Q * UNIT).astype(F32), 1.5 * UNIT, 8)
    labels, sizes, n_neighbors, core = lattice_oracle(Q, 1.5, 8)
    assert 0.2 < core.mean() < 0.8 and ((labels >= 0) & ~core).sum() > 1000 and (labels < 0).sum() > 1000 and len(sizes) > 10
    assert np.array_equal(got.n_neighbors, n_neighbors) and np.array_equal(got.core, core)
    assert np.array_equal(got.sizes, sizes)
    # the partition through a label bijection: every pair (ours, oracle's) that occurs pairs one label with one label, noise with noise
    seen = np.unique(np.stack([got.labels, labels], axis=1), axis=0)
    assert len(seen) == len(np.unique(seen[:, 0])) == len(np.unique(seen[:, 1])) and (seen[seen[:, 0] < 0] == -1).all()
    assert np.array_equal(got.labels, labels)                              # and the numbering itself
    assert (sizes == 12 ** 3).sum() == 3                                   # each blob whole: its corners are border points of it


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------------------
def test_one_point(gpu):
    one = np.array([[0.25, -1.0, 3.0]], F32)
    got = _run(one, 0.1, 1)
    assert got.labels.tolist() == [0] and got.sizes.tolist() == [1] and got.n_neighbors.tolist() == [1] and got.core.tolist() == [True]
    got = _run(one, 0.1, 2)
    assert got.labels.tolist() == [-1] and got.sizes.shape == (0,) and got.n_neighbors.tolist() == [1] and got.core.tolist() == [False]


def test_no_valid_point_and_no_point(gpu):
    bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]], F32)
    got = _run(bad, 0.1, 1)
    assert got.labels.tolist() == [-1] * 3 and got.sizes.shape == (0,) and got.n_neighbors.tolist() == [0] * 3 and not got.core.any()
    got = _run(np.zeros((0, 3), F32), 0.1, 1)
    assert got.labels.shape == (0,) and got.sizes.shape == (0,) and got.core.dtype == bool


def test_identical_points_are_one_cluster(gpu):
    P = np.tile(np.array([[1.5, 2.5, -0.5]], F32), (300, 1))
    got = _run(P, 0.01, 10)
    assert got.sizes.tolist() == [300] and (got.labels == 0).all() and (got.n_neighbors == 300).all() and got.core.all()
    got = _run(P, 0.01, 301)
    assert got.sizes.shape == (0,) and (got.labels == -1).all() and (got.n_neighbors == 300).all()


def test_min_points_above_every_neighbourhood_is_all_noise(gpu):
    got = _run(SCENE, 0.08, 10 ** 6)
    want = scene_restated(0.08, 6)
    assert got.sizes.shape == (0,) and got.sizes.dtype == np.int32 and (got.labels == -1).all() and not got.core.any()
    assert np.array_equal(got.n_neighbors, want.n_neighbors)


def test_ranges_that_leave_the_grid(gpu):
    """eps far above the cloud's extent: every padded range leaves the grid on all six sides and is clamped to it; and eps so far below it
    that the cell has to be doubled to fit 21 bits per axis. Neither changes what is found."""
    rng = np.random.default_rng(31)
    P = rng.random((700, 3)).astype(F32)
    P[50:60] = P[40:50]                                                    # duplicates: the only neighbours at the tiny radius
    P[100] = np.nan
    for eps, min_points in ((50.0, 5), (0.9, 650), (3e-8, 2), (0.06, 3)):
        _same(_run(P, eps, min_points), restated_dbscan(P, eps, min_points))
    far = np.concatenate([P, [[1e6, 1e6, 1e6], [-1e6, 0, 0]]]).astype(F32)  # two far points stretch the grid; the rest shares a few cells
    _same(_run(far, 0.06, 3), restated_dbscan(far, 0.06, 3))


# ---- 4. one walk: the search and the clustering look at the same points --------------------------------------------------------------------
def walk_cloud(r):
    """(308, 3) float32: the reference lattice of test_cloud_metrics_cpu.lattice_case (spacing r, side 6, with its 20 duplicates) plus its
    72 queries one and two spacings outside every face, so that the padded ranges of the inner points are cut at those of the outer ones
    and those of the outer ones leave the grid; a NaN, a +inf and a -inf row"""
    Q, R = lattice_case(np.random.default_rng(21), r, 0.0, side=6)
    assert len(Q) == 30 + 12 * (12 + 6) + 30 + 20                          # lattice_case's layout: per (axis, k) 12 displaced sites, then 6 beyond the face
    beyond = Q[30:30 + 12 * 18].reshape(12, 18, 3)[:, 12:].reshape(-1, 3)
    P = np.concatenate([R, beyond]).astype(F32)
    P[3, 0], P[100, 1], P[-1, 2] = np.nan, np.inf, -np.inf
    return P


@pytest.mark.parametrize('factor', [0.5, 1.0, 2.0])
def test_search_and_clustering_walk_the_same_points(gpu, factor):
    """d3r_cloud_nearest, d3r_cloud_knn and d3r_cloud_cluster on ONE grid of the cloud, the cloud as its own queries: per point the same
    number of distance evaluations, that of the numpy restatement of the walk, and zero at the non-finite rows; and the clustering's
    n_neighbors is the number of columns a 32-column search fills (every point here has fewer than 32 neighbours: on a lattice of spacing r
    the sites within r are the point's own and its six axis neighbours, each held once or a few times)."""
    import ctypes as C
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from dust3r_amd.cloud_metrics import _bounds
    from dust3r_amd.viz import fuse_key_bits
    for r in (0.25, 1e-3):
        P = walk_cloud(r)
        n, bad = len(P), ~np.isfinite(P).all(axis=1)
        assert bad.sum() == 3
        cell = np.float32(r) * np.float32(factor)
        want_evals = restated_grid_nearest(P, P, r, cell)[2]
        want_count = restated_dbscan(P, r, 1).n_neighbors                   # the fp32 brute force over all pairs
        assert want_count.max() < 32 and want_count[~bad].min() >= 1 and (want_evals[bad] == 0).all() and (want_evals[~bad] >= want_count[~bad]).all()
        Pd = torch.from_numpy(P).to(gpu)
        i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=gpu)      # noqa: E731
        with torch.cuda.device(gpu):
            lo, hi, n_valid = _bounds(Pd, gpu)
            assert n_valid == n - 3
            lo_c, bits_c = (C.c_float * 3)(*lo.tolist()), (C.c_int * 3)(*fuse_key_bits(lo, hi, cell))
            grid = torch.empty(int(lib.d3r_cloud_grid_workspace_bytes(n, n)), dtype=torch.uint8, device=gpu)
            work = torch.empty(int(lib.d3r_cloud_cluster_workspace_bytes(n)), dtype=torch.uint8, device=gpu)
            where = (lo_c, float(cell), bits_c)
            check(lib.d3r_cloud_grid_build(n, ptr(Pd), *where, ptr(grid), current_stream()), 'build')
            ev_nearest, ev_knn, ev_cluster = i32(n), i32(n), i32(n)
            d2 = {k: torch.empty((n, k), device=gpu) for k in (1, 8, 32)}
            idx = {k: i32(n, k) for k in (1, 8, 32)}
            radius, stream = float(np.float32(r)), current_stream()
            check(lib.d3r_cloud_nearest(n, n, ptr(Pd), radius, *where, 0, ptr(d2[1]), ptr(idx[1]), ptr(ev_nearest), ptr(grid), stream), 'nearest')
            check(lib.d3r_cloud_knn(n, n, ptr(Pd), 8, radius, *where, 0, 0, ptr(d2[8]), ptr(idx[8]), ptr(ev_knn), ptr(grid), stream), 'knn')
            check(lib.d3r_cloud_knn(n, n, ptr(Pd), 32, radius, *where, 0, 0, ptr(d2[32]), ptr(idx[32]), None, ptr(grid), stream), 'knn at k = 32')
            labels, sizes, n_clusters, n_neighbors, core = i32(n), i32(n), i32(1), i32(n), torch.zeros((n,), dtype=torch.uint8, device=gpu)
            check(lib.d3r_cloud_cluster(n, radius, 4, *where, ptr(labels), ptr(sizes), ptr(n_clusters), ptr(n_neighbors), ptr(core), ptr(ev_cluster), None,
                                        ptr(grid), ptr(work), stream), 'cluster')
        ev_nearest, ev_knn, ev_cluster = (t.cpu().numpy() for t in (ev_nearest, ev_knn, ev_cluster))
        assert np.array_equal(ev_nearest, ev_knn) and np.array_equal(ev_knn, ev_cluster), r
        assert np.array_equal(ev_cluster, want_evals) and (ev_cluster[bad] == 0).all() and ev_cluster.max() > 0, r
        filled = torch.isfinite(d2[32]).sum(dim=1).cpu().numpy()
        assert np.array_equal(n_neighbors.cpu().numpy(), filled) and np.array_equal(filled, want_count), r


# ---- 5. through the API -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene(gpu):
    from test_fuse_gpu import _scene
    return _scene(gpu, 3, 24, 32, 5)


def _with_blob(cloud):
    """the fused cloud plus a planted floater: a flat 8 x 8 patch sampled at 0.7 voxels, 30 voxels beyond the cloud's corner -- as dense as the
    surface, which is what the statistical outlier removal cannot tell from it"""
    from dust3r_amd.viz import FusedCloud
    v = cloud.voxel_size
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), indexing='ij'), axis=-1).reshape(-1, 2)
    blob = (np.asarray(cloud.bounds[1], np.float64) + 30 * v + np.c_[0.7 * v * g, np.zeros(len(g))]).astype(F32)
    m = len(blob)
    out = FusedCloud(np.concatenate([cloud.positions, blob]), np.concatenate([cloud.colors, np.full((m, 3), 200, np.uint8)]),
                     np.concatenate([cloud.weight, np.ones(m, F32)]), np.concatenate([cloud.count, np.ones(m, np.int32)]), v,
                     (cloud.bounds[0], blob.max(axis=0)))
    return out, np.arange(len(out)) >= len(cloud)


def test_cluster_and_keep_clusters_remove_a_floater_that_outlier_removal_keeps(gpu, scene):
    cloud, is_blob = _with_blob(scene.fuse())
    clustered = cloud.cluster()
    assert clustered.labels.shape == (len(cloud),) and clustered.labels.dtype == np.int32 and clustered.positions is cloud.positions
    assert np.array_equal(np.bincount(clustered.labels[clustered.labels >= 0]), clustered.cluster_sizes)
    by_hand = _run(cloud.positions, 2.5 * cloud.voxel_size, 10)           # the default: eps = 2.5 voxels, min_points = 10
    assert np.array_equal(by_hand.labels, clustered.labels) and np.array_equal(by_hand.sizes, clustered.cluster_sizes)
    blob_label = set(clustered.labels[is_blob].tolist())
    assert len(blob_label) == 1 and blob_label != {-1}                     # the blob is one cluster ...
    assert not (clustered.labels[~is_blob] == blob_label.pop()).any()      # ... of its own ...
    assert clustered.cluster_sizes[0] > is_blob.sum() and clustered.labels[is_blob][0] > 0      # ... and not the largest
    kept, keep = clustered.keep_clusters(largest=1)
    assert not keep[is_blob].any() and keep.sum() == clustered.cluster_sizes[0] == len(kept) and (kept.labels == 0).all()
    _, survives = cloud.remove_outliers()                                  # the gap this closes: at its defaults the blob stays
    assert survives[is_blob].all()
    plain, _ = clustered.remove_outliers()
    assert np.array_equal(plain.labels, clustered.labels[survives])        # labels follow the points that stay
    explicit = cloud.cluster(eps=2.5 * cloud.voxel_size, min_points=10)
    assert np.array_equal(explicit.labels, clustered.labels)
    coloured = clustered.colored_by_label()
    assert coloured.colors.shape == cloud.colors.shape and coloured.colors.dtype == np.uint8


def test_scene_fuse_with_clusters_and_its_untouched_defaults(gpu, scene, tmp_path):
    from dust3r_amd.export import read_ply
    a, b = scene.fuse(), scene.fuse(clusters=None, keep_largest=None)
    assert a.labels is None and a.cluster_sizes is None
    for name in ('positions', 'colors', 'weight', 'count'):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes()
    full = scene.fuse(clusters=True)
    assert len(full) == len(a) and full.labels.shape == (len(a),) and np.array_equal(full.labels, a.cluster().labels)
    wide = scene.fuse(clusters=dict(eps=4 * a.voxel_size, min_points=5))
    assert np.array_equal(wide.labels, a.cluster(eps=4 * a.voxel_size, min_points=5).labels)
    cloud = scene.fuse(clusters=True, keep_largest=1, normals=True, tracks=True)
    m = len(cloud)
    assert 0 < m == full.cluster_sizes[0] and (cloud.labels == 0).all() and np.array_equal(cloud.cluster_sizes, full.cluster_sizes)
    assert cloud.normals.shape == (m, 3) and cloud.curvature.shape == (m,) and cloud.colors.shape == (m, 3) and cloud.weight.shape == (m,)
    assert cloud.tracks.n_points == m
    assert np.array_equal(read_ply(cloud.save_ply(str(tmp_path / 'c.ply')))['label'], cloud.labels)
    assert np.array_equal(scene.fuse(keep_largest=1).positions, cloud.positions)      # keep_largest alone implies the clustering
    with pytest.raises(ValueError, match='clusters'):
        scene.fuse(clusters=dict(radius=1.0))
    dev = scene.fuse(clusters=True, to_host=False)
    assert dev.labels.is_cuda and dev.cluster_sizes.is_cuda and np.array_equal(dev.labels.cpu().numpy(), full.labels)
    kept, keep = dev.keep_clusters(largest=1)
    assert keep.is_cuda and int(keep.sum()) == len(kept) == m


def test_demo_writer_labels_the_ply_and_reports_the_clusters(gpu, scene, tmp_path):
    """the demo's writer (what --fuse_clusters / --fuse_keep_largest reach): scene.ply carries the labels, cameras.json the cluster count and
    the ten largest sizes"""
    import copy
    import json
    from dust3r_amd import demo
    from dust3r_amd.export import read_ply
    demo.write_cameras(str(tmp_path), scene)
    written = demo.write_fused(str(tmp_path), copy.deepcopy(scene), min_conf_thr=1.0, clusters=0.0)
    ply = read_ply(written[0])
    doc = json.load(open(str(tmp_path / 'cameras.json')))
    sizes = np.bincount(ply['label'][ply['label'] >= 0])
    assert doc['clusters']['count'] == len(sizes) > 0 and doc['clusters']['largest'] == sizes[:10].tolist() and doc['clusters']['kept'] is None
    assert 'cam2world' in doc and 'tracks' not in doc
    written = demo.write_fused(str(tmp_path), copy.deepcopy(scene), min_conf_thr=1.0, clusters=4.0, keep_largest=1, normals=True)
    kept = read_ply(written[0])
    doc = json.load(open(str(tmp_path / 'cameras.json')))
    assert (kept['label'] == 0).all() and len(kept['label']) == doc['clusters']['largest'][0] and doc['clusters']['kept'] == 1
    assert kept['normals'].shape == kept['positions'].shape
    plain = read_ply(demo.write_fused(str(tmp_path), copy.deepcopy(scene), min_conf_thr=1.0)[0])
    assert 'label' not in plain
