"""The k nearest neighbours, normals and outlier removal of the fused cloud, without a GPU: PLY with normals, the demo's flags, the outlier
threshold, and the numpy restatements that tests/test_cloud_knn_gpu.py holds the kernels of csrc/cloud_knn.hip against, checked here
against each other.
- `brute_force_knn`: THE definition (include/dust3r_hip.h, d3r_cloud_knn): chunked fp32 numpy over all pairs, d2 = (dx dx + dy dy) + dz dz
  with every operation rounded on its own, the candidates d2 <= r r, np.lexsort on (index, d2), the first k, padded with (+inf, -1).
- `restated_means` / `restated_threshold`: the mean neighbour distances (sequential fp64 sum of np.sqrt in column order, one rounding) and
  mean + ratio std (sample std) of the full rows.
- `restated_normals`: np.linalg.eigh in fp64 on the scatter matrix of the point and its found neighbours.
- `restated_orientation`: the visibility vote, projection in fp32 in the kernel's operation order, the vote in fp64."""
import math
import os

import numpy as np
import pytest

from test_cloud_metrics_cpu import brute_force, valid_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def brute_force_knn(Q, R, k, r, exclude_self=False, chunk=128):
    """(d2 (n, k) float32, idx (n, k) int32) of the definition"""
    Q, R, r = np.asarray(Q, F32).reshape(-1, 3), np.asarray(R, F32).reshape(-1, 3), F32(r)
    r2 = r * r
    rows = np.flatnonzero(valid_rows(R))
    Rv = R[rows]
    d2_out, idx_out = np.full((len(Q), k), np.inf, F32), np.full((len(Q), k), -1, np.int32)
    if len(Rv) == 0:
        return d2_out, idx_out
    kk = min(k, len(Rv))
    for s in range(0, len(Q), chunk):
        q = Q[s:s + chunk]
        ok = valid_rows(q)
        with np.errstate(over='ignore', invalid='ignore'):
            d = np.where(ok[:, None], q, F32(0))[:, None, :] - Rv[None, :, :]
            m = d * d
            d2 = (m[..., 0] + m[..., 1]) + m[..., 2]
        assert d2.dtype == F32
        cand = ok[:, None] & (d2 <= r2)
        if exclude_self:
            cand &= rows[None, :] != (s + np.arange(len(q)))[:, None]
        key = np.where(cand, d2, F32(np.inf))
        order = np.lexsort((np.broadcast_to(rows, key.shape), key), axis=1)[:, :kk]      # by d2, then by index
        take = np.take_along_axis(cand, order, axis=1)                                   # candidates come first: d2 <= r2 < inf
        d2_out[s:s + chunk, :kk] = np.where(take, np.take_along_axis(d2, order, axis=1), F32(np.inf))
        idx_out[s:s + chunk, :kk] = np.where(take, rows[order], -1)
    return d2_out, idx_out


def restated_means(d2, idx):
    """(mean (n,) float32, NaN where a row is short; full (n,) bool): the fp64 sum of np.sqrt in column order, divided by k, one rounding"""
    full = (idx >= 0).all(axis=1)
    s = np.zeros(len(d2), np.float64)
    with np.errstate(invalid='ignore'):
        for j in range(d2.shape[1]):
            s = s + np.sqrt(d2[:, j].astype(np.float64))
        mean = np.where(full, s / d2.shape[1], np.nan).astype(F32)
    return mean, full


def restated_threshold(means, std_ratio):
    """mean + std_ratio std (sample std, as Open3D) of the fp32 means widened to fp64"""
    m = np.asarray(means, np.float64)
    return float(m.mean() + std_ratio * (m.std(ddof=1) if len(m) > 1 else 0.0))


def lead_positive(v):
    """rows of v signed so that the first component of largest magnitude is positive"""
    lead = np.take_along_axis(v, np.abs(v).argmax(axis=1)[:, None], axis=1)
    return np.where(lead < 0, -v, v)


def restated_normals(P, R, idx, min_neighbors=3):
    """(normals (n, 3) fp64, curvature (n,) fp64, eigenvalues (n, 3), found (n,)) by np.linalg.eigh on the scatter matrix of the point
    followed by its found neighbours; zero normal and NaN curvature below min_neighbors"""
    P, R = np.asarray(P, np.float64), np.asarray(R, np.float64)
    n = len(P)
    normals, curv, lam = np.zeros((n, 3)), np.full(n, np.nan), np.full((n, 3), np.nan)
    found = (idx >= 0).sum(axis=1)
    for q in np.flatnonzero(found >= min_neighbors):
        sample = np.concatenate([P[q:q + 1], R[idx[q][idx[q] >= 0]]])
        c = sample - sample.mean(axis=0)
        w, v = np.linalg.eigh(c.T @ c)
        normals[q], lam[q], curv[q] = v[:, 0], w, w[0] / w.sum()
    return lead_positive(normals), curv, lam, found


def restated_orientation(P, N, depth, conf, K, w2c, centers, shapes, tol):
    """(n_seen (n,) int, s (n,) fp64 the vote, sum_w (n,) fp64, seen (n, views) bool, cosines (n, views) fp64). depth, conf: lists of
    (h, w) maps. The projection in fp32, left to right, as the kernel; the vote in fp64 in view order."""
    P, N = np.asarray(P, F32), np.asarray(N, F32)
    n, nv = len(P), len(depth)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    seen, cosines, weights = np.zeros((n, nv), bool), np.zeros((n, nv)), np.zeros((n, nv))
    tol = F32(tol)
    with np.errstate(all='ignore'):
        for v in range(nv):
            M, Kv = np.asarray(w2c[v], F32), np.asarray(K[v], F32)
            px, py, pz = (((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3))
            ku, kv, kw = ((Kv[r, 0] * px + Kv[r, 1] * py) + Kv[r, 2] * pz for r in range(3))
            assert pz.dtype == F32 and kw.dtype == F32
            uu, vv = np.rint(ku / kw), np.rint(kv / kw)
            h, w = shapes[v]
            inside = (pz > 0) & (uu >= 0) & (uu < w) & (vv >= 0) & (vv < h)
            ui, vi = np.where(inside, uu, 0).astype(np.int64), np.where(inside, vv, 0).astype(np.int64)
            d = np.asarray(depth[v], F32)[vi, ui]
            seen[:, v] = inside & (np.abs(pz - d) <= tol * d)
            weights[:, v] = np.asarray(conf[v], F32)[vi, ui].astype(np.float64)
            dx, dy, dz = (np.float64(centers[v][c]) - P[:, c].astype(np.float64) for c in range(3))
            length = np.sqrt(dx * dx + dy * dy + dz * dz)
            dot = N[:, 0].astype(np.float64) * dx + N[:, 1].astype(np.float64) * dy + N[:, 2].astype(np.float64) * dz
            cosines[:, v] = np.where(length > 0, dot / length, 0.0)
    n_seen = seen.sum(axis=1)
    s, sum_w = np.zeros(n), np.zeros(n)
    for v in range(nv):
        wv = np.where(n_seen > 0, np.where(seen[:, v], weights[:, v], 0.0), 1.0)
        s = s + wv * cosines[:, v]
        sum_w = sum_w + wv
    return n_seen, s, sum_w, seen, cosines


# ---- the restatements against each other ------------------------------------------------------------------------------------------------
def test_brute_force_knn_is_the_single_neighbour_definition_at_k_1_and_sorted_beyond():
    rng = np.random.default_rng(1)
    R = rng.random((700, 3)).astype(F32)
    R[::2] = R[1::2]                                                   # every point twice: d2 = 0 ties
    R[5::97, 1] = np.nan
    Q = rng.random((300, 3)).astype(F32)
    Q[::41, 0] = np.inf
    one = brute_force_knn(Q, R, 1, 0.1)
    want = brute_force(Q, R, 0.1)
    assert np.array_equal(one[0][:, 0], want[0]) and np.array_equal(one[1][:, 0], want[1])
    d2, idx = brute_force_knn(R, R, 9, 0.15, exclude_self=True)
    ok = valid_rows(R)
    assert (idx[~ok] == -1).all() and np.isinf(d2[~ok]).all() and (idx[ok, 0] >= 0).all()
    assert (idx != np.arange(len(R))[:, None]).all()                   # never the query's own index ...
    twins = ok.reshape(-1, 2).all(axis=1).repeat(2)
    assert (d2[twins, 0] == 0).all()                                   # ... its twin at the other index stays
    pairs = np.stack([d2[:, :-1], d2[:, 1:]])
    both = idx[:, 1:] >= 0
    assert ((pairs[0] < pairs[1]) | ((pairs[0] == pairs[1]) & (idx[:, :-1] < idx[:, 1:])))[both].all()      # ascending (d2, index)
    assert ((idx[:, :-1] >= 0) | (idx[:, 1:] < 0)).all()               # the padding comes last
    assert 0 < (idx[:, -1] < 0).sum() < len(R)


def test_outlier_threshold_is_the_restated_one():
    from dust3r_amd.cloud_metrics import outlier_threshold
    rng = np.random.default_rng(2)
    means = (0.02 + 0.005 * rng.random(3000)).astype(F32)
    means[::50] *= F32(4)
    m = means.astype(np.float64)
    for ratio in (0.5, 2.0, 3.0):
        got = outlier_threshold(len(m), math.fsum(m), math.fsum(m * m), ratio)
        want = restated_threshold(means, ratio)
        assert abs(got - want) <= 1e-12 * want
    assert math.isnan(outlier_threshold(0, 0.0, 0.0, 2.0))
    assert outlier_threshold(1, 0.25, 0.0625, 2.0) == 0.25
    assert outlier_threshold(4, 2.0, 1.0 - 1e-12, 2.0) == 0.5          # a variance that rounds below zero counts as zero
    mean, full = restated_means(np.array([[1, 4], [1, np.inf]], F32), np.array([[0, 1], [0, -1]], np.int32))
    assert mean[0] == 1.5 and np.isnan(mean[1]) and full.tolist() == [True, False]


def test_restated_normals_on_a_sphere_are_radial():
    rng = np.random.default_rng(3)
    P = rng.standard_normal((600, 3))
    P = (P / np.linalg.norm(P, axis=1, keepdims=True)).astype(F32)
    d2, idx = brute_force_knn(P, P, 12, 0.5, exclude_self=True)
    normals, curv, lam, found = restated_normals(P, P, idx)
    assert (found == 12).all() and (np.abs(np.linalg.norm(normals, axis=1) - 1) < 1e-12).all()
    assert (np.abs((normals * P).sum(axis=1)) > 0.98).all() and (curv < 0.05).all() and (lam[:, 0] <= lam[:, 1]).all()
    lead = np.take_along_axis(normals, np.abs(normals).argmax(axis=1)[:, None], axis=1)
    assert (lead > 0).all()


# ---- PLY --------------------------------------------------------------------------------------------------------------------------------
def _cloud_arrays(n, seed=4):
    rng = np.random.default_rng(seed)
    normals = rng.standard_normal((n, 3)).astype(F32)
    return ((rng.random((n, 3)) * 5 - 2).astype(F32), rng.integers(0, 256, (n, 3)).astype(np.uint8), (rng.random(n) * 9).astype(F32),
            rng.integers(1, 40, n).astype(np.int32), normals / np.linalg.norm(normals, axis=1, keepdims=True).astype(F32))


def test_ply_with_normals_round_trips(tmp_path):
    from dust3r_amd.export import read_ply, write_ply
    pos, col, wgt, cnt, nrm = _cloud_arrays(257)
    path = write_ply(str(tmp_path / 'n.ply'), pos, col, wgt, cnt, normals=nrm)
    header = open(path, 'rb').read().split(b'end_header\n')[0].decode('ascii').split('\n')
    props = [ln.split()[-1] for ln in header if ln.startswith('property ')]
    assert props == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue', 'confidence', 'count']      # nx ny nz directly after z
    back = read_ply(path)
    assert sorted(back) == ['colors', 'confidence', 'count', 'normals', 'positions']
    for got, want in ((back['positions'], pos), (back['colors'], col), (back['confidence'], wgt), (back['count'], cnt), (back['normals'], nrm)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    bare = read_ply(write_ply(str(tmp_path / 'bare.ply'), pos, col, normals=nrm))       # normals without confidence / count
    assert sorted(bare) == ['colors', 'normals', 'positions'] and np.array_equal(bare['normals'], nrm)
    empty = read_ply(write_ply(str(tmp_path / 'empty.ply'), pos[:0], col[:0], wgt[:0], cnt[:0], normals=nrm[:0]))
    assert empty['normals'].shape == (0, 3) and empty['normals'].dtype == F32


def test_ply_without_normals_keeps_its_bytes(tmp_path):
    from dust3r_amd.export import read_ply, write_ply
    pos, col, wgt, cnt, _ = _cloud_arrays(100)
    a = open(write_ply(str(tmp_path / 'a.ply'), pos, col, wgt, cnt), 'rb').read()
    b = open(write_ply(str(tmp_path / 'b.ply'), pos, col, wgt, cnt, normals=None), 'rb').read()
    assert a == b and b'nx' not in a.split(b'end_header')[0]
    assert len(a) == a.index(b'end_header\n') + len(b'end_header\n') + 100 * (12 + 3 + 4 + 4)      # the layout of the four-argument call
    assert 'normals' not in read_ply(str(tmp_path / 'a.ply'))


def test_ply_normals_of_another_length_raise(tmp_path):
    from dust3r_amd.export import write_ply
    pos, col, wgt, cnt, nrm = _cloud_arrays(50)
    with pytest.raises(ValueError, match='normals of shape'):
        write_ply(str(tmp_path / 'x.ply'), pos, col, wgt, cnt, normals=nrm[:49])
    with pytest.raises(ValueError, match='normals of shape'):
        write_ply(str(tmp_path / 'x.ply'), pos, col, wgt, cnt, normals=nrm[:, :2])


def test_fused_cloud_carries_normals_through_save_ply(tmp_path):
    from dust3r_amd.export import read_ply
    from dust3r_amd.viz import FusedCloud
    pos, col, wgt, cnt, nrm = _cloud_arrays(64)
    plain = FusedCloud(pos, col, wgt, cnt, 0.1, (pos.min(axis=0), pos.max(axis=0)))
    assert plain.normals is None and plain.curvature is None
    assert 'normals' not in read_ply(plain.save_ply(str(tmp_path / 'plain.ply')))
    curv = np.linspace(0, 0.3, 64).astype(F32)
    cloud = FusedCloud(pos, col, wgt, cnt, 0.1, (pos.min(axis=0), pos.max(axis=0)), normals=nrm, curvature=curv)
    back = read_ply(cloud.save_ply(str(tmp_path / 'normals.ply')))
    assert np.array_equal(back['normals'], nrm) and np.array_equal(back['positions'], pos) and np.array_equal(back['count'], cnt)
    assert cloud.curvature is curv and len(cloud) == 64


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_demo_flags_imply_fuse():
    from dust3r_amd.demo import get_args_parser, wants_fuse
    parse = lambda *extra: get_args_parser().parse_args(['pics', '--weights', 'w.pth', *extra])      # noqa: E731
    plain = parse()
    assert plain.fuse_normals is False and plain.fuse_outliers is None and not wants_fuse(plain)
    a = parse('--fuse_normals')
    assert a.fuse_normals is True and a.fuse is None and wants_fuse(a)
    b = parse('--fuse_outliers', '2.5')
    assert b.fuse_outliers == 2.5 and b.fuse_normals is False and wants_fuse(b)
    assert wants_fuse(parse('--fuse_outliers', '0'))                   # a ratio of zero is a request too
    for old in (('--fuse',), ('--ply',), ('--colmap',), ('--fuse', '0.01')):
        assert wants_fuse(parse(*old))
    with pytest.raises(SystemExit):
        parse('--fuse_outliers')                                       # the ratio is required
