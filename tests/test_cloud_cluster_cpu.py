"""Density clustering of the fused cloud (DBSCAN) without a GPU: the numpy restatement that tests/test_cloud_cluster_gpu.py holds
csrc/cloud_cluster.hip against, pinned here on a scene with known structure, and the host-side parts of the feature.
- `restated_dbscan`: THE definition (include/dust3r_hip.h, d3r_cloud_cluster): an fp32 all-pairs adjacency d2 = (dx dx + dy dy) + dz dz <=
  eps eps, the point itself a neighbour; core = at least min_points neighbours; scipy's connected_components on the core graph, rooted at
  the lowest index; border points to the core neighbour of smallest (d2, index); clusters numbered by decreasing size, ties by root.
- `make_scene`: a bumpy sheet, a sphere, a thin bridge that stops short of the sphere, two blobs, uniform noise, exact duplicates, one NaN
  and one Inf row, permuted on a fixed seed.
- argument checks of cluster_points / FusedCloud.cluster / keep_clusters / write_ply, the PLY label property, the demo's new flags, the
  build's resource report."""
import collections
import os
import re

import numpy as np
import pytest

F32 = np.float32
Restated = collections.namedtuple('Restated', 'labels sizes n_neighbors core roots')


def restated_dbscan(P, eps, min_points):
    """labels (n,) int32, sizes (C,) int32, n_neighbors (n,) int32, core (n,) bool, roots (n,) int64 (the lowest core index of the point's
    cluster, -1 for noise) of the definition; O(n^2) memory, for clouds of a few thousand points"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    P = np.asarray(P, F32)
    n = len(P)
    valid = np.isfinite(P).all(axis=1)
    eps2 = F32(eps) * F32(eps)
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy, dz = (P[:, None, c] - P[None, :, c] for c in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz                                 # fp32, every operation rounded on its own
    assert d2.dtype == F32
    adj = (d2 <= eps2) & valid[:, None] & valid[None, :]
    n_neighbors = adj.sum(axis=1).astype(np.int32)
    core = valid & (n_neighbors >= min_points)
    roots = np.full(n, -1, np.int64)
    core_idx = np.nonzero(core)[0]
    if len(core_idx):
        n_comp, comp = connected_components(csr_matrix(adj[np.ix_(core_idx, core_idx)]), directed=False)
        comp_root = np.full(n_comp, n, np.int64)
        np.minimum.at(comp_root, comp, core_idx)
        roots[core_idx] = comp_root[comp]
        masked = np.where(adj & core[None, :], d2, F32(np.inf))           # the core neighbours' distances
        nearest = np.argmin(masked, axis=1)                                # the first minimum: the lowest index of minimal d2
        border = valid & ~core & np.isfinite(masked[np.arange(n), nearest])
        roots[border] = roots[nearest[border]]
    labels = np.full(n, -1, np.int32)
    uniq, sizes = np.unique(roots[roots >= 0], return_counts=True)
    order = np.lexsort((uniq, -sizes))
    rank = np.empty(len(uniq), np.int64)
    rank[order] = np.arange(len(uniq))
    labels[roots >= 0] = rank[np.searchsorted(uniq, roots[roots >= 0])]
    return Restated(labels, sizes[order].astype(np.int32), n_neighbors, core, roots)


def make_scene(seed=1, side=1.7):
    """(2318, 3) float32: sheet 1200, sphere 500, bridge 400, blobs 40 and 6, noise 150, 20 duplicates, a NaN row, an Inf row; permuted"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.0, side, (1200, 2))
    sheet = np.c_[xy, 0.05 * np.sin(4 * xy[:, 0]) * np.cos(3 * xy[:, 1])]
    u = rng.standard_normal((500, 3))
    centre, radius = np.array([3.0, 1.0, 0.6]), 0.28
    sphere = centre + radius * u / np.linalg.norm(u, axis=1, keepdims=True)
    t = np.sort(rng.uniform(0.0, 1.0, 400))
    start, stop = np.array([3.0, 1.0, 2.2]), centre + np.array([0.0, 0.0, radius + 0.08])      # above the sphere's top, 0.08 short of it
    bridge = start + t[:, None] * (stop - start) + rng.normal(0.0, 0.004, (400, 3))
    blob40 = np.array([1.0, 3.0, 1.0]) + rng.normal(0.0, 0.02, (40, 3))
    blob6 = np.array([2.0, 3.0, 1.5]) + rng.normal(0.0, 0.01, (6, 3))
    noise = rng.uniform([-0.5, -0.5, -0.5], [4.0, 3.5, 2.5], (150, 3))
    P = np.concatenate([sheet, sphere, bridge, blob40, blob6, noise])
    P = np.concatenate([P, P[rng.choice(len(P), 20, replace=False)], [[np.nan, 0.5, 0.5]], [[0.5, np.inf, 0.5]]])
    return P[rng.permutation(len(P))].astype(F32)


SCENE = make_scene()
PARAMS = [(0.08, 6), (0.12, 10), (0.05, 4)]
_restated = {}


def scene_restated(eps, min_points):
    """the restatement on SCENE, computed once per parameter pair and shared (tests/test_cloud_cluster_gpu.py reads it too)"""
    key = (eps, min_points)
    if key not in _restated:
        _restated[key] = restated_dbscan(SCENE, eps, min_points)
    return _restated[key]


def partition_of(labels):
    """the clusters as a set of frozensets of point indices: what a labelling means, whatever its numbering"""
    labels = np.asarray(labels)
    return {frozenset(np.nonzero(labels == c)[0].tolist()) for c in np.unique(labels[labels >= 0])}


# ---- 1. the scene, pinned -------------------------------------------------------------------------------------------------------------------
def test_scene_is_the_described_one():
    assert SCENE.shape == (2318, 3) and SCENE.dtype == F32
    valid = np.isfinite(SCENE).all(axis=1)
    assert (~valid).sum() == 2 and np.isnan(SCENE).any(axis=1).sum() == 1 and np.isinf(SCENE).any(axis=1).sum() == 1
    assert len(SCENE) - len(np.unique(SCENE[valid], axis=0)) - 2 == 20      # the exact duplicates
    assert np.array_equal(SCENE, make_scene(), equal_nan=True)              # a fixed seed


def test_restatement_on_the_scene_gives_the_pinned_clusters():
    """The structure the scene was built for: at (0.08, 6) the sheet, the sphere, the bridge and both blobs are clusters of their own (the
    bridge stops 0.08 short of the sphere) next to one small clump of noise and duplicates; at (0.12, 10) the bridge has joined the sphere
    and the 6-point blob is noise; at (0.05, 4) the sheet and the sphere break up. The numbers are those of this generator and seed."""
    valid = np.isfinite(SCENE).all(axis=1)
    r = scene_restated(0.08, 6)
    assert r.sizes.tolist() == [1186, 504, 406, 40, 8, 6]
    assert int(((r.labels >= 0) & ~r.core).sum()) == 111 and int(((r.labels < 0) & valid).sum()) == 166
    assert int(r.sizes.sum()) + 166 == int(valid.sum()) == 2316
    r = scene_restated(0.12, 10)
    assert r.sizes.tolist() == [1210, 910, 40]
    r = scene_restated(0.05, 4)
    assert len(r.sizes) == 100 and r.sizes[0] == 406 and (np.diff(r.sizes) <= 0).all()


@pytest.mark.parametrize('eps,min_points', PARAMS)
def test_restatement_keeps_the_rules(eps, min_points):
    r = scene_restated(eps, min_points)
    valid = np.isfinite(SCENE).all(axis=1)
    assert (r.labels[~valid] == -1).all() and (r.n_neighbors[~valid] == 0).all() and not r.core[~valid].any()
    assert (r.n_neighbors[valid] >= 1).all()                               # the point itself
    assert (r.labels[r.core] >= 0).all()
    assert np.array_equal(np.bincount(r.labels[r.labels >= 0], minlength=len(r.sizes)), r.sizes)
    for c in range(len(r.sizes)):                                          # the root is the lowest CORE index of the cluster
        members = np.nonzero(r.labels == c)[0]
        assert (r.roots[members] == members[r.core[members]].min()).all()
    # duplicates share a label: equal coordinates have equal neighbourhoods, and equal (d2, index) choices
    _, inverse, counts = np.unique(SCENE[valid], axis=0, return_inverse=True, return_counts=True)
    twins = np.nonzero(valid)[0][counts[inverse.ravel()] > 1]
    assert len(twins) == 40
    for i in twins:
        same = np.nonzero((SCENE == SCENE[i]).all(axis=1))[0]
        assert len(set(r.labels[same].tolist())) == 1 and len(set(r.core[same].tolist())) == 1


def test_partition_does_not_depend_on_the_order_of_the_points():
    eps, min_points = 0.08, 6
    r = scene_restated(eps, min_points)
    perm = np.random.default_rng(3).permutation(len(SCENE))
    q = restated_dbscan(SCENE[perm], eps, min_points)
    back = np.empty_like(q.labels)
    back[perm] = q.labels                                                  # the permuted run's labels in the original order
    assert partition_of(back) == partition_of(r.labels) and np.array_equal(q.sizes, r.sizes)
    assert np.array_equal(q.core, r.core[perm]) and np.array_equal(q.n_neighbors, r.n_neighbors[perm])


def test_min_points_of_one_makes_every_valid_point_core():
    r = restated_dbscan(SCENE, 0.08, 1)
    valid = np.isfinite(SCENE).all(axis=1)
    assert np.array_equal(r.core, valid) and np.array_equal(r.labels >= 0, valid)


def test_equal_sizes_are_numbered_by_root():
    """two clusters of five points each: the one that holds the lower index comes first, whichever way round they are stored"""
    a = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0.1, 0.1, 0], [0.05, 0.05, 0]], F32)
    b = a + F32(10)
    for first, second in ((a, b), (b, a)):
        r = restated_dbscan(np.concatenate([first, second, [[50, 50, 50]]]).astype(F32), 0.2, 3)
        assert r.sizes.tolist() == [5, 5] and r.labels.tolist() == [0] * 5 + [1] * 5 + [-1]
        assert r.roots.tolist() == [0] * 5 + [5] * 5 + [-1]
    mixed = np.concatenate([b[:1], a, b[1:]]).astype(F32)                  # b holds index 0: it is cluster 0
    assert restated_dbscan(mixed, 0.2, 3).labels.tolist() == [0] + [1] * 5 + [0] * 4


def test_border_point_goes_to_the_nearest_core_neighbour_then_to_the_lower_index():
    """a point between two clusters: nearer to the right one; then at equal distances, where the lower index decides"""
    left = np.array([[-1.0, 0, 0], [-1.1, 0, 0], [-1.2, 0, 0], [-1.05, 0.05, 0]], F32)
    right = -left
    for x, want in ((0.02, 'right'), (-0.02, 'left'), (0.0, 'lower')):      # within 1.03 of both (+-1, 0, 0), and of nothing else
        P = np.concatenate([[[x, 0, 0]], right, left]).astype(F32)         # indices: 0 the border point, 1-4 right, 5-8 left
        r = restated_dbscan(P, 1.03, 4)
        assert r.n_neighbors[0] == 3
        assert not r.core[0] and r.core[1:].all()
        assert r.roots[0] == {'right': 1, 'left': 5, 'lower': 1}[want]


# ---- 2. argument checks: before the device is touched ---------------------------------------------------------------------------------------
def _fused(n=12, voxel=0.1, **kw):
    from dust3r_amd.viz import FusedCloud
    rng = np.random.default_rng(0)
    pos = rng.random((n, 3)).astype(F32)
    return FusedCloud(pos, rng.integers(0, 256, (n, 3)).astype(np.uint8), np.ones(n, F32), np.ones(n, np.int32), voxel, (pos.min(axis=0), pos.max(axis=0)), **kw)


def test_cluster_points_checks_its_arguments_first():
    from dust3r_amd.cloud_metrics import cluster_points
    P = SCENE[:10]
    for eps in (0.0, -1.0, float('nan'), float('inf'), 1e-30, 1e30):
        with pytest.raises(ValueError, match='eps'):
            cluster_points(P, eps)
    for bad in (0, -3, 2.5, True, None, '4'):
        with pytest.raises(ValueError, match='min_points'):
            cluster_points(P, 0.1, min_points=bad)


def test_fused_cloud_cluster_checks_its_arguments_first():
    with pytest.raises(ValueError, match='no voxel size'):
        _fused(voxel=float('nan')).cluster()
    with pytest.raises(ValueError, match='eps'):
        _fused().cluster(eps=0.0)
    with pytest.raises(ValueError, match='min_points'):
        _fused().cluster(min_points=0)


def test_keep_clusters_takes_exactly_one_selector():
    labels, sizes = np.array([0, 0, 0, 1, 1, -1, 2, 0, 1, 2, -1, 0], np.int32), np.array([5, 3, 2], np.int32)
    cloud = _fused(labels=labels, cluster_sizes=sizes, normals=np.ones((12, 3), F32), curvature=np.zeros(12, F32))
    for kw in ({}, dict(largest=1, min_size=2), dict(largest=1, labels=[0]), dict(largest=1, min_size=1, labels=[0])):
        with pytest.raises(ValueError, match='exactly one'):
            cloud.keep_clusters(**kw)
    for kw in (dict(largest=-1), dict(largest=1.5), dict(min_size=0), dict(labels=[3]), dict(labels=[-1]), dict(labels=[0.5])):
        with pytest.raises(ValueError, match='keep_clusters'):
            cloud.keep_clusters(**kw)
    with pytest.raises(ValueError, match='no labels'):
        _fused().keep_clusters(largest=1)
    kept, keep = cloud.keep_clusters(largest=2)
    assert np.array_equal(keep, (labels == 0) | (labels == 1)) and len(kept) == 8 and kept.tracks is None
    assert np.array_equal(kept.labels, labels[keep]) and kept.cluster_sizes is sizes and kept.normals.shape == (8, 3) and kept.curvature.shape == (8,)
    assert np.array_equal(cloud.keep_clusters(min_size=3)[1], keep)
    assert np.array_equal(cloud.keep_clusters(labels=[2, 0])[1], (labels == 0) | (labels == 2))
    assert not cloud.keep_clusters(largest=0)[1].any() and np.array_equal(cloud.keep_clusters(largest=9)[1], labels >= 0)


def test_label_colors_are_a_fixed_palette_and_grey_for_noise():
    from dust3r_amd.viz import LABEL_NOISE_COLOR, LABEL_PALETTE, label_colors
    labels = np.array([0, 1, 19, 20, 41, -1], np.int32)
    col = label_colors(labels)
    assert col.shape == (6, 3) and col.dtype == np.uint8 and LABEL_PALETTE.shape == (20, 3)
    assert np.array_equal(col[:5], LABEL_PALETTE[[0, 1, 19, 0, 1]]) and tuple(col[5]) == LABEL_NOISE_COLOR == (128, 128, 128)
    assert len({tuple(c) for c in LABEL_PALETTE.tolist()}) == 20 and LABEL_NOISE_COLOR not in {tuple(c) for c in LABEL_PALETTE.tolist()}
    cloud = _fused(6, labels=labels, cluster_sizes=np.zeros(42, np.int32)).colored_by_label()
    assert np.array_equal(cloud.colors, col) and cloud.labels is labels
    with pytest.raises(ValueError, match='no labels'):
        _fused().colored_by_label()


def test_fused_cloud_carries_labels_where_the_points_stay():
    labels, sizes = np.arange(12, dtype=np.int32) % 3, np.array([4, 4, 4], np.int32)
    cloud = _fused(labels=labels, cluster_sizes=sizes)
    assert cloud.labels is labels and cloud.cluster_sizes is sizes
    plain = _fused()
    assert plain.labels is None and plain.cluster_sizes is None


FIELDS = ('positions', 'colors', 'weight', 'count', 'voxel_size', 'bounds', 'normals', 'curvature', 'tracks', 'labels', 'cluster_sizes')


def test_derived_clouds_keep_carry_or_drop_every_field():
    """every deriving method that runs without a GPU, on a cloud with ALL eleven fields set, field by field as the docstrings say: kept (the
    same object), carried along (the masked rows) or dropped (None); origin follows bounds"""
    import inspect
    from dust3r_amd.viz import FusedCloud
    assert tuple(inspect.signature(FusedCloud.__init__).parameters)[1:] == FIELDS
    assert set(FusedCloud.PER_POINT) == {'positions', 'colors', 'weight', 'count', 'normals', 'curvature', 'labels'}
    rng = np.random.default_rng(4)
    labels, sizes, tracks = np.array([0, 0, 0, 1, 1, -1, 2, 0, 1, 2, -1, 0], np.int32), np.array([5, 3, 2], np.int32), object()
    cloud = _fused(normals=rng.random((12, 3)).astype(F32), curvature=rng.random(12).astype(F32), tracks=tracks, labels=labels, cluster_sizes=sizes)
    assert all(getattr(cloud, name) is not None for name in FIELDS) and cloud.origin is cloud.bounds[0]

    coloured = cloud.colored_by_label()                                    # the same points: only the colours are new
    assert coloured is not cloud and coloured.colors is not cloud.colors and coloured.colors.shape == (12, 3)
    for name in FIELDS:
        if name != 'colors':
            assert getattr(coloured, name) is getattr(cloud, name) or name == 'voxel_size' and coloured.voxel_size == cloud.voxel_size, name
    assert coloured.origin is cloud.bounds[0]

    kept, keep = cloud.keep_clusters(largest=1)                            # a subset: rows carried along, tracks dropped, the rest kept
    assert np.array_equal(keep, labels == 0) and len(kept) == 5
    for name in FusedCloud.PER_POINT:
        assert np.array_equal(getattr(kept, name), getattr(cloud, name)[keep]) and getattr(kept, name).dtype == getattr(cloud, name).dtype, name
    assert kept.tracks is None and kept.cluster_sizes is sizes and kept.bounds is cloud.bounds and kept.origin is cloud.bounds[0]
    assert kept.voxel_size == cloud.voxel_size
    for name in FIELDS:                                                    # and the cloud it came from is as it was
        assert getattr(cloud, name) is not None, name
    assert cloud.tracks is tracks and cloud.labels is labels

    bare, _ = _fused(labels=labels, cluster_sizes=sizes).keep_clusters(min_size=3)      # what the cloud does not have stays None
    assert bare.normals is None and bare.curvature is None and bare.tracks is None and len(bare.labels) == 8


# ---- 3. PLY ----------------------------------------------------------------------------------------------------------------------------------
def test_ply_with_labels_round_trips(tmp_path):
    from dust3r_amd.export import read_ply, write_ply
    rng = np.random.default_rng(5)
    n = 77
    pos, col = rng.random((n, 3)).astype(F32), rng.integers(0, 256, (n, 3)).astype(np.uint8)
    wgt, cnt, nrm = rng.random(n).astype(F32), rng.integers(1, 9, n).astype(np.int32), rng.standard_normal((n, 3)).astype(F32)
    labels = rng.integers(-1, 5, n).astype(np.int32)
    path = write_ply(str(tmp_path / 'l.ply'), pos, col, wgt, cnt, normals=nrm, labels=labels)
    header = open(path, 'rb').read().split(b'end_header\n')[0].decode('ascii').split('\n')
    assert [ln.split()[1:] for ln in header if ln.startswith('property ')][-3:] == [['float', 'confidence'], ['int', 'count'], ['int', 'label']]
    back = read_ply(path)
    assert sorted(back) == ['colors', 'confidence', 'count', 'label', 'normals', 'positions']
    assert back['label'].dtype == np.int32 and np.array_equal(back['label'], labels) and np.array_equal(back['count'], cnt)
    bare = read_ply(write_ply(str(tmp_path / 'bare.ply'), pos, col, labels=labels.astype(np.int64)))
    assert sorted(bare) == ['colors', 'label', 'positions'] and np.array_equal(bare['label'], labels)
    cloud = _fused(labels=np.arange(12, dtype=np.int32) - 1, cluster_sizes=np.ones(11, np.int32))
    assert np.array_equal(read_ply(cloud.save_ply(str(tmp_path / 'c.ply')))['label'], np.arange(12) - 1)
    with pytest.raises(ValueError, match='label'):
        write_ply(str(tmp_path / 'x.ply'), pos, col, labels=labels[:-1])
    with pytest.raises(ValueError, match='labels are integers'):
        write_ply(str(tmp_path / 'x.ply'), pos, col, labels=labels.astype(F32))
    assert not os.path.exists(str(tmp_path / 'x.ply'))


def test_ply_without_labels_keeps_its_bytes(tmp_path):
    """against bytes put together by hand: the header and the packed rows of the file as it was before the label property existed"""
    from dust3r_amd.export import read_ply, write_ply
    rng = np.random.default_rng(6)
    n = 33
    pos, col = rng.random((n, 3)).astype(F32), rng.integers(0, 256, (n, 3)).astype(np.uint8)
    wgt, cnt = rng.random(n).astype(F32), rng.integers(1, 9, n).astype(np.int32)
    header = ('ply\nformat binary_little_endian 1.0\ncomment dust3r_amd fused cloud\nelement vertex 33\nproperty float x\nproperty float y\n'
              'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty float confidence\nproperty int count\n'
              'end_header\n').encode('ascii')
    body = b''.join(pos[i].astype('<f4').tobytes() + col[i].tobytes() + wgt[i:i + 1].astype('<f4').tobytes() + cnt[i:i + 1].astype('<i4').tobytes()
                    for i in range(n))
    assert len(body) == n * 23
    for kw in ({}, dict(labels=None)):
        assert open(write_ply(str(tmp_path / 'p.ply'), pos, col, wgt, cnt, **kw), 'rb').read() == header + body
    assert open(_plain_cloud(pos, col, wgt, cnt).save_ply(str(tmp_path / 'q.ply')), 'rb').read() == header + body
    assert 'label' not in read_ply(str(tmp_path / 'p.ply'))


def _plain_cloud(pos, col, wgt, cnt):
    from dust3r_amd.viz import FusedCloud
    return FusedCloud(pos, col, wgt, cnt, 0.1, (pos.min(axis=0), pos.max(axis=0)))


# ---- 4. the command line and scene.fuse's arguments -------------------------------------------------------------------------------------------
def test_demo_cluster_flags_imply_fuse():
    from dust3r_amd.demo import get_args_parser, wants_fuse
    parse = lambda *extra: get_args_parser().parse_args(['pics', '--weights', 'w.pth', *extra])      # noqa: E731
    plain = parse()
    assert plain.fuse_clusters is None and plain.fuse_keep_largest is None and not wants_fuse(plain)
    a = parse('--fuse_clusters')
    assert a.fuse_clusters == 0.0 and a.fuse is None and wants_fuse(a)     # 0: the default eps of FusedCloud.cluster
    b = parse('--fuse_clusters', '3.5')
    assert b.fuse_clusters == 3.5 and wants_fuse(b)
    c = parse('--fuse_keep_largest', '2')
    assert c.fuse_keep_largest == 2 and c.fuse_clusters is None and wants_fuse(c)
    with pytest.raises(SystemExit):
        parse('--fuse_keep_largest')
    with pytest.raises(SystemExit):
        parse('--fuse_keep_largest', '1.5')


def test_library_exports_the_clustering():
    from dust3r_amd._lib import EXPORTED, lib
    assert {'d3r_cloud_cluster', 'd3r_cloud_cluster_workspace_bytes'} <= set(EXPORTED)
    assert lib.d3r_cloud_cluster_workspace_bytes(0) == 0 and lib.d3r_cloud_cluster_workspace_bytes(-5) == 0
    small, large = lib.d3r_cloud_cluster_workspace_bytes(1), lib.d3r_cloud_cluster_workspace_bytes(10 ** 6)
    assert 0 < small < large and large >= 10 ** 6 * (2 * 8 + 2 * 4 + 4 + 4 + 1 + 2 * 8 + 2 * 4)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'dust3r_hip.h')).read()
    assert 'int d3r_cloud_cluster(int n, float eps, int min_points' in header and 'size_t d3r_cloud_cluster_workspace_bytes(int n);' in header


def test_c_entry_refuses_bad_arguments_without_a_launch():
    """D3R_ERR_INVALID comes back before any HIP call: the checks run on a machine without a GPU"""
    import ctypes as C
    from dust3r_amd._lib import lib
    lo, bits, one = (C.c_float * 3)(0, 0, 0), (C.c_int * 3)(4, 4, 4), C.c_void_p(256)
    good = dict(n=8, eps=0.5, min_points=3, lo=lo, cell=0.5, bits=bits, labels=one, sizes=one, n_clusters=one, n_neighbors=one, core=one, evals=None,
                events=None, grid=one, work=one, stream=None)
    call = lambda **kw: lib.d3r_cloud_cluster(*dict(good, **kw).values())      # noqa: E731
    bad_bits = (C.c_int * 3)(4, 22, 4)
    for kw in (dict(n=0), dict(n=-1), dict(eps=0.0), dict(eps=float('nan')), dict(eps=1e-30), dict(eps=1e30), dict(min_points=0), dict(lo=None),
               dict(bits=None), dict(bits=bad_bits), dict(cell=0.0), dict(labels=None), dict(sizes=None), dict(n_clusters=None), dict(n_neighbors=None),
               dict(core=None), dict(grid=None), dict(work=None)):
        assert call(**kw) != 0, kw


# ---- 5. the resource report ---------------------------------------------------------------------------------------------------------------
def test_resource_report_has_no_scratch():
    """read only: the report is what the build left next to the object; nothing is built or touched here"""
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'cloud_cluster.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no cloud_cluster.resources.txt: the library was not built by dust3r_amd/build.py')
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    new = [k for k in kernels if 'cluster_' in k]
    assert len(new) == 8 and all('cluster_' in k or 'cloud_' in k or 'fuse_' in k for k in kernels)
    assert sum('fuse_flag_kernel' in k for k in kernels) == 6             # KEYS, HEADS and ROOTS, counting and placing (fuse_grid.hpp)
    for name in ('cluster_count_kernel', 'cluster_union_kernel', 'cluster_border_kernel', 'cluster_flatten_kernel'):
        assert sum(name in k for k in new) == 1
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
