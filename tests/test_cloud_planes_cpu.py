"""Plane detection (csrc/cloud_planes.hip; cloud_metrics.plane_ransac / segment_plane / detect_planes): the numpy restatement of the
definitions of include/dust3r_hip.h, tested on its own here and compared with the kernels by tests/test_cloud_planes_gpu.py, and the
host pieces (plane_from_moments, ground_plane, upright_similarity, the argument checks, the PLY property). No GPU.

The restatement computes every fp32 and fp64 operation with numpy scalars or arrays of that type, one rounding each, in the order the
header writes them; the sampler is `restated_samples` of tests/test_cloud_global_cpu.py. The support's sums are math.fsum of the same
terms: the correctly rounded sum, from which a sum in any order lies within (n - 1) 2^-53 sum |term|.

PLANTED is a scene with known answers: a floor of 20 x 15 lattice points at spacing 0.125 on y = 0.5, a wall of 14 x 12 lattice points on
x = 2.5 (y from 0.625), 131 clutter points uniform in [0, 2.5)^3, all permuted. Lattice coordinates are exact in fp32, so a sample of
three floor points gives the normal (0, +-1, 0) and d = -+0.5 without any rounding, and many hypotheses tie for the best count: the
lowest-h rule decides."""
import math

import numpy as np
import pytest

from dust3r_amd.cloud_metrics import (Plane, Planes, default_plane_min_inliers, detect_planes, ground_plane, moments_covariance, plane_centre,
                                      plane_from_moments, plane_ransac, plane_rms, plane_support, segment_plane, transform_planes, upright_similarity)
from test_cloud_global_cpu import restated_samples
from test_cloud_metrics_cpu import valid_rows

F32 = np.float32
THR, MIN_AREA2 = 0.01, 0.01


# ---- 1. the restatement -------------------------------------------------------------------------------------------------------------------
def restated_plane_hypotheses(P, seed, n_hyp, min_area2):
    """(planes (H, 4) float64, valid (H,) bool) of d3r_plane_ransac's hypotheses"""
    P = np.asarray(P, F32)
    pick = restated_samples(seed, n_hyp, len(P))
    ok = pick[:, 2] >= 0
    i = np.where(pick < 0, 0, pick)
    ok &= valid_rows(P)[i].all(axis=1)
    p0, p1, p2 = (P[i[:, c]].astype(np.float64) for c in range(3))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        u, v = p1 - p0, p2 - p0
        c = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        l = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        ok &= l >= min_area2
        n = c / l[:, None]
        d = -((n[:, 0] * p0[:, 0] + n[:, 1] * p0[:, 1]) + n[:, 2] * p0[:, 2])
        planes = np.concatenate([n, d[:, None]], axis=1)
        ok &= np.isfinite(planes).all(axis=1)
    return np.where(ok[:, None], planes, 0.0), ok


def restated_residual(row, P):
    """e = ((nx x + ny y) + nz z) + d in fp32 for the fp32 row (4,)"""
    row, P = np.asarray(row, F32), np.asarray(P, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        return ((row[0] * P[:, 0] + row[1] * P[:, 1]) + row[2] * P[:, 2]) + row[3]


def restated_inliers(row, P, thr, normals=None, cos_min=0.0):
    """(n,) bool: THE INLIER TEST of include/dust3r_hip.h for the fp32 row"""
    row, P = np.asarray(row, F32), np.asarray(P, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        inl = valid_rows(P) & (np.abs(restated_residual(row, P)) <= F32(thr))
        if normals is not None:
            N = np.asarray(normals, F32)
            cos = (row[0] * N[:, 0] + row[1] * N[:, 1]) + row[2] * N[:, 2]
            inl &= np.isfinite(N).all(axis=1) & (N != 0).any(axis=1) & (np.abs(cos) >= F32(cos_min))
    return inl


def _f32(planes):
    with np.errstate(over='ignore'):
        return np.asarray(planes, np.float64).astype(F32)


def restated_plane_ransac(P, seed, n_hyp, thr, normals=None, cos_min=0.0, min_area2=None, min_inliers=3):
    """dict(h, count, n_valid, model (4,) float64, inliers (n,) bool, counts (H,) with -1 for invalid hypotheses): d3r_plane_ransac"""
    P = np.asarray(P, F32)
    min_area2 = (8.0 * float(F32(thr))) ** 2 if min_area2 is None else min_area2
    planes, valid = restated_plane_hypotheses(P, seed, n_hyp, min_area2)
    rows = _f32(planes)
    counts = np.full(n_hyp, -1, np.int64)
    for h in np.flatnonzero(valid):
        counts[h] = restated_inliers(rows[h], P, thr, normals, cos_min).sum()
    h = int(np.argmax(counts)) if valid.any() else -1                              # the first of equal counts
    if h < 0 or counts[h] < min_inliers:
        return dict(h=-1, count=0, n_valid=int(valid.sum()), model=np.zeros(4), inliers=np.zeros(len(P), bool), counts=counts)
    return dict(h=h, count=int(counts[h]), n_valid=int(valid.sum()), model=planes[h], inliers=restated_inliers(rows[h], P, thr, normals, cos_min),
                counts=counts)


def moment_terms(P, mask, centre):
    """(count, 9) float64: the terms of d3r_plane_support's sums for the points of the mask"""
    a = np.asarray(P, F32)[mask].astype(np.float64) - np.asarray(centre, F32).astype(np.float64)
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    return np.stack([x, y, z, x * x, x * y, x * z, y * y, y * z, z * z], axis=1)


def restated_support(P, plane, thr, centre, normals=None, cos_min=0.0):
    """(mask (n,) bool, count, sums (9,) float64 by math.fsum, sum |term| (9,)): d3r_plane_support of float32(plane)"""
    mask = restated_inliers(_f32(plane), P, thr, normals, cos_min)
    terms = moment_terms(P, mask, centre)
    return mask, int(mask.sum()), np.array([math.fsum(col) for col in terms.T]), np.abs(terms).sum(axis=0)


def restated_segment(P, thr, n_hyp=4096, normals=None, cos_min=0.0, min_area2=None, min_inliers=3, seed=0, refine_rounds=3):
    """cloud_metrics.segment_plane: dict(model, inliers, count, rms, rounds, ransac, thr) or None; rounds = per support pass (model, count, sums, sum
    |term|, centre): every plane whose mask was taken, the RANSAC winner first"""
    best = restated_plane_ransac(P, seed, n_hyp, thr, normals, cos_min, min_area2, min_inliers)
    if best['h'] < 0:
        return None
    model = best['model'].copy()
    centre = plane_centre(model)
    previous, rounds = None, []
    for r in range(refine_rounds + 1):
        mask, count, sums, mags = restated_support(P, model, thr, centre, normals, cos_min)
        rounds.append(dict(model=model, count=count, sums=sums, mags=mags, centre=centre))
        if r == refine_rounds or count == previous:
            break
        refit = plane_from_moments(count, sums, centre)
        if refit is None or not np.isfinite(_f32(refit)).all():
            break
        model, previous = refit, count
    return dict(model=model, inliers=mask, count=count, rms=plane_rms(model, count, sums, centre), rounds=rounds, ransac=best, thr=thr)


def restated_detect(P, thr, max_planes=6, min_inliers=None, n_hyp=4096, normals=None, cos_min=0.0, min_area2=None, seed=0, refine_rounds=3):
    """cloud_metrics.detect_planes: (planes (P, 4), sizes (P,) int32, labels (n,) int32, the `restated_segment` of every round and its rows)"""
    P = np.asarray(P, F32)
    min_inliers = default_plane_min_inliers(len(P)) if min_inliers is None else min_inliers
    labels = np.full(len(P), -1, np.int32)
    rows = np.arange(len(P))
    planes, sizes, segments = [], [], []
    for r in range(max_planes):
        if len(rows) < 3:
            break
        seg = restated_segment(P[rows], thr, n_hyp, None if normals is None else np.asarray(normals, F32)[rows], cos_min, min_area2, min_inliers,
                               seed + r, refine_rounds)
        if seg is None or seg['count'] < min_inliers:
            break
        labels[rows[seg['inliers']]] = r
        planes.append(seg['model'])
        sizes.append(seg['count'])
        segments.append((seg, rows))
        rows = rows[~seg['inliers']]
    return np.array(planes, np.float64).reshape(-1, 4), np.array(sizes, np.int32), labels, segments


def gate_margin(seg, P, thr):
    """how near, in fp64, any finite point comes to |e| = thr for any plane whose mask `restated_segment` took"""
    P64 = np.asarray(P, F32).astype(np.float64)[valid_rows(P)]
    return min(float(np.abs(np.abs(P64 @ _f32(r['model'])[:3].astype(np.float64) + float(_f32(r['model'])[3])) - float(F32(thr))).min())
               for r in seg['rounds'])


# ---- 2. the planted scene -------------------------------------------------------------------------------------------------------------------
def planted():
    """(points (599, 3) float32, kind (599,): 0 floor, 1 wall, 2 clutter)"""
    rng = np.random.default_rng(0)
    i, j = np.meshgrid(np.arange(20), np.arange(15), indexing='ij')
    floor = np.stack([0.125 * i.ravel(), np.full(i.size, 0.5), 0.125 * j.ravel()], axis=1)
    i, j = np.meshgrid(np.arange(14), np.arange(12), indexing='ij')
    wall = np.stack([np.full(i.size, 2.5), 0.625 + 0.125 * i.ravel(), 0.125 * j.ravel()], axis=1)
    clutter = rng.uniform(0, 2.5, (131, 3))
    pts = np.concatenate([floor, wall, clutter]).astype(F32)
    kind = np.repeat([0, 1, 2], [len(floor), len(wall), len(clutter)])
    order = rng.permutation(len(pts))
    return pts[order], kind[order]


PLANTED, KIND = planted()


def test_the_planted_scene_is_the_one_described():
    assert PLANTED.shape == (599, 3) and PLANTED.dtype == F32 and np.bincount(KIND).tolist() == [300, 168, 131]
    assert (PLANTED[KIND == 0][:, 1] == 0.5).all() and (PLANTED[KIND == 1][:, 0] == 2.5).all() and PLANTED[KIND == 1][:, 1].min() == 0.625


@pytest.mark.parametrize('n_hyp', [64, 300, 513])
@pytest.mark.parametrize('seed', [0, 1, 2, 3])
def test_restated_ransac_finds_the_floor_exactly_and_breaks_ties_by_the_lowest_hypothesis(seed, n_hyp):
    best = restated_plane_ransac(PLANTED, seed, n_hyp, THR, min_area2=MIN_AREA2)
    assert best['inliers'][KIND == 0].all() and best['count'] == best['inliers'].sum() >= 300
    n, d = best['model'][:3], best['model'][3]
    assert np.array_equal(np.abs(n), [0.0, 1.0, 0.0]) and d == -0.5 * n[1]                  # exactly: lattice coordinates
    ties = np.flatnonzero(best['counts'] == best['count'])
    assert len(ties) >= 2 and best['h'] == ties[0]                                     # a condition on the input: the rule is exercised
    assert 0 < best['n_valid'] <= n_hyp and best['n_valid'] == (best['counts'] >= 0).sum()


@pytest.mark.parametrize('n_hyp', [64, 513])
@pytest.mark.parametrize('seed', [0, 3])
def test_restated_detect_takes_the_floor_then_the_wall(seed, n_hyp):
    planes, sizes, labels, segments = restated_detect(PLANTED, THR, max_planes=2, min_inliers=100, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=seed)
    assert len(planes) == 2 and sizes.dtype == np.int32 and labels.dtype == np.int32
    assert (labels[KIND == 0] == 0).all() and (labels[KIND == 1] == 1).all()
    assert sizes[0] == (labels == 0).sum() >= 300 and sizes[1] == (labels == 1).sum() == 168
    assert abs(abs(planes[0][1]) - 1) < 1e-4 and abs(abs(planes[1][0]) - 1) < 1e-12 and abs(planes[1][3] + 2.5 * planes[1][0]) < 1e-12
    assert segments[1][0]['rms'] < 1e-12 and segments[0][0]['rms'] < THR
    for seg, rows in segments:
        assert gate_margin(seg, PLANTED[rows], THR) > 1e-5
    third = restated_detect(PLANTED, THR, max_planes=6, min_inliers=100, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=seed)
    assert len(third[0]) == 2 and np.array_equal(third[2], labels)                     # the clutter holds no plane of 100 points: it stops


def test_restated_segment_refits_and_stops_when_the_count_stays():
    seg = restated_segment(PLANTED, THR, n_hyp=64, min_area2=MIN_AREA2, seed=0)
    assert 2 <= len(seg['rounds']) <= 4 and seg['rounds'][0]['count'] == seg['ransac']['count']
    assert np.array_equal(seg['rounds'][0]['model'], seg['ransac']['model'])
    assert seg['count'] == seg['inliers'].sum() and seg['inliers'][KIND == 0].all()
    e = PLANTED[seg['inliers']].astype(np.float64) @ seg['model'][:3] + seg['model'][3]
    assert abs(seg['rms'] - math.sqrt((e * e).mean())) < 1e-12                         # the rms from the moments is the rms of the residuals
    none = restated_segment(PLANTED, THR, n_hyp=64, min_area2=MIN_AREA2, min_inliers=400)
    assert none is None
    plain = restated_segment(PLANTED, THR, n_hyp=64, min_area2=MIN_AREA2, refine_rounds=0)
    assert len(plain['rounds']) == 1 and np.array_equal(plain['model'], seg['ransac']['model'])


def test_restated_normals_gate():
    N = np.zeros_like(PLANTED)
    N[KIND == 0] = (0, -1, 0)                                                          # the sign does not matter
    N[KIND == 1] = (1, 0, 0)
    N[KIND == 2] = (0, 0, 1)
    floor = np.flatnonzero(KIND == 0)
    N[floor[0]] = 0                                                                    # no normal: not an inlier, whatever cos_min
    N[floor[1]] = (np.nan, 1, 0)
    for cos_min in (0.9, 0.0, -1.0):
        best = restated_plane_ransac(PLANTED, 0, 64, THR, N, cos_min, MIN_AREA2)
        assert best['count'] == (298 if cos_min > 0 else 300) and not best['inliers'][floor[:2]].any() and best['inliers'][floor[2:]].all()


# ---- 3. the host pieces -----------------------------------------------------------------------------------------------------------------------
def test_plane_from_moments_is_the_least_squares_plane():
    rng = np.random.default_rng(4)
    n = np.array([0.3, -0.9, 0.2])
    n /= np.linalg.norm(n)
    basis = np.linalg.svd(n[None])[2][1:]
    pts = (rng.uniform(-2, 2, (500, 2)) @ basis + 1.7 * n + 1e-3 * rng.standard_normal((500, 1)) * n).astype(F32)
    centre = np.array([0.5, -1.5, 0.25], F32)
    terms = moment_terms(pts, np.ones(500, bool), centre)
    sums = terms.sum(axis=0)
    model = plane_from_moments(500, sums, centre)
    assert abs(np.linalg.norm(model[:3]) - 1) < 1e-15 and model[1] > 0 and abs(model[1]) == np.abs(model[:3]).max()      # the sign rule
    assert np.abs(model[:3] + n).max() < 1e-3 and abs(model[3] - 1.7) < 1e-3
    p64 = pts.astype(np.float64)
    _, vec = np.linalg.eigh(np.cov(p64.T, bias=True))
    assert abs(abs(vec[:, 0] @ model[:3]) - 1) < 1e-12 and abs(model[:3] @ p64.mean(axis=0) + model[3]) < 1e-12
    e = p64 @ model[:3] + model[3]
    assert abs(plane_rms(model, 500, sums, centre) - math.sqrt((e * e).mean())) < 1e-12
    mean, cov = moments_covariance(500, sums)
    assert np.abs(mean + centre - p64.mean(axis=0)).max() < 1e-12 and np.abs(cov - np.cov(p64.T, bias=True)).max() < 1e-12
    assert plane_from_moments(2, sums, centre) is None and plane_from_moments(500, sums * np.nan, centre) is None
    assert np.array_equal(plane_centre([0, 1, 0, -0.5]), np.array([0, 0.5, 0], F32))


def test_ground_plane_takes_the_largest_plane_with_every_camera_on_one_side():
    planes = np.array([[1.0, 0, 0, -2.5], [0, -1.0, 0, 0.5], [0, 0, 1.0, -1.0]])
    cams = np.array([[1.0, 1.5, 0.5], [2.0, 1.2, 1.5], [3.0, 1.4, 0.7]])                  # above the floor, on both sides of x = 2.5
    g = ground_plane(planes, [900, 300, 50], cams, 0.01)
    assert np.array_equal(g, [0, 1.0, 0, -0.5])                                        # the sign turned towards the cameras
    assert np.array_equal(ground_plane(planes, [900, 300, 50], cams[:, [0, 2, 1]], 0.01), [0, 0, 1.0, -1.0])      # y and z swapped: a camera on y = 0.5
    assert ground_plane(planes[:1], [900], cams, 0.01) is None
    assert ground_plane(planes[1:2], [300], cams, 1.0) is None                         # a camera within thr of the plane: no side
    assert ground_plane(np.zeros((0, 4)), [], cams, 0.01) is None
    tie = ground_plane(np.array([[0, 1.0, 0, -0.5], [0, 1.0, 0, -0.25]]), [10, 10], cams, 0.01)
    assert tie[3] == -0.5                                                              # the first of equal supports
    with pytest.raises(ValueError):
        ground_plane(planes, [1, 2], cams, 0.01)


def test_upright_similarity_levels_the_planted_floor():
    R0 = upright_similarity([0.6, 0.0, 0.8, 0.3])[:3, :3]
    T0 = np.eye(4)
    T0[:3, :3] = R0.T                                                                  # any rotation: tilt the scene with it
    T0[:3, 3] = (0.3, -1.1, 2.0)
    floor = PLANTED[KIND == 0].astype(np.float64) @ T0[:3, :3].T + T0[:3, 3]
    plane = transform_planes([[0, 1.0, 0, -0.5]], T0)[0]
    assert np.abs(floor @ plane[:3] + plane[3]).max() < 1e-12
    for model in (plane, -plane, 3.0 * plane):
        T = upright_similarity(model)
        moved = floor @ T[:3, :3].T + T[:3, 3]
        assert np.abs(moved[:, 1]).max() <= 1e-6
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(T[:3, :3]) - 1) <= 1e-12
        assert np.array_equal(T[3], [0, 0, 0, 1])
        n = model[:3] / np.linalg.norm(model[:3])
        assert np.abs(T[:3, :3] @ n - [0, 1, 0]).max() <= 1e-12
        angle = math.degrees(math.acos(min(1.0, (np.trace(T[:3, :3]) - 1) / 2)))
        assert abs(angle - math.degrees(math.acos(n[1]))) < 1e-6                       # the least angle: the one between n and up
    assert np.array_equal(upright_similarity([0, 2.0, 0, -1.0]), np.array([[1.0, 0, 0, 0], [0, 1, 0, -0.5], [0, 0, 1, 0], [0, 0, 0, 1]]))
    flip = upright_similarity([0, -1.0, 0, 0.5])                                       # half a turn
    assert np.abs(flip[:3, :3] @ [0, -1.0, 0] - [0, 1, 0]).max() <= 1e-12 and abs(flip[1, 3] - 0.5) <= 1e-12
    z = upright_similarity([0, 1.0, 0, -0.5], up=(0, 0, 1))
    assert np.abs(z[:3, :3] @ [0, 1.0, 0] - [0, 0, 1]).max() <= 1e-12
    with pytest.raises(ValueError):
        upright_similarity([0, 0, 0, 1.0])


def test_transform_planes_follows_a_similarity():
    from test_cloud_icp_cpu import similarity
    S = similarity((1, -2, 0.5), 50.0, 1.8, (0.2, 3.0, -1.0))
    pts = PLANTED[KIND == 1].astype(np.float64)
    moved = pts @ S[:3, :3].T + S[:3, 3]
    plane = transform_planes([[1.0, 0, 0, -2.5]], S)[0]
    assert abs(np.linalg.norm(plane[:3]) - 1) < 1e-12 and np.abs(moved @ plane[:3] + plane[3]).max() < 1e-12


# ---- 4. arguments -----------------------------------------------------------------------------------------------------------------------------
def test_host_entry_points_check_their_arguments_before_the_device():
    P = np.zeros((4, 3), F32)
    bad = (dict(thr=0.0), dict(thr=-1.0), dict(thr=float('nan')), dict(thr=float('inf')), dict(thr=1e39), dict(n_hyp=0), dict(n_hyp=2 ** 23 + 1),
           dict(n_hyp=1.5), dict(cos_min=float('nan')), dict(min_area2=0.0), dict(min_area2=float('nan')), dict(min_inliers=2), dict(min_inliers=2.5))
    for kw in bad:
        for f in (plane_ransac, segment_plane, detect_planes):
            with pytest.raises(ValueError):
                f(P, **dict(dict(thr=0.1), **kw))
    for kw in (dict(refine_rounds=-1), dict(refine_rounds=1.5)):
        for f in (segment_plane, detect_planes):
            with pytest.raises(ValueError):
                f(P, 0.1, **kw)
    with pytest.raises(ValueError):
        detect_planes(P, 0.1, max_planes=-1)
    for kw in (dict(thr=0.0), dict(plane=[0, 1, 0, np.inf]), dict(centre=[np.nan, 0, 0]), dict(cos_min=float('nan'))):
        with pytest.raises(ValueError):
            plane_support(P, **dict(dict(plane=[0, 1, 0, 0], thr=0.1, centre=[0, 0, 0]), **kw))
    assert Plane._fields == ('model', 'inliers', 'count', 'rms') and Planes._fields == ('planes', 'plane_sizes', 'plane_labels')
    assert default_plane_min_inliers(10) == 3 and default_plane_min_inliers(1000) == 20


def test_exports_refuse_bad_arguments_without_a_launch():
    import ctypes as C
    from dust3r_amd._lib import EXPORTED, lib
    assert {'d3r_plane_ransac', 'd3r_plane_ransac_workspace_bytes', 'd3r_plane_support', 'd3r_plane_support_workspace_bytes'} <= set(EXPORTED)
    wb = lib.d3r_plane_ransac_workspace_bytes
    assert wb(2, 16) == 0 and wb(3, 0) == 0 and wb(3, 2 ** 23 + 1) == 0 and wb(3, 1) >= 4 * 8 + 12 * 4 + 8
    assert wb(3, 4096) == wb(100000, 4096) and wb(3, 2 ** 20) >= 2 ** 20 * (4 * 8 + 12 * 4 + 8)
    sb = lib.d3r_plane_support_workspace_bytes
    assert sb(0) == 0 and sb(-1) == 0 and sb(1) >= 10 * 8 and sb(10 ** 7) <= 1024 * 10 * 8 + 256
    one = C.c_void_p(256)                                                              # never dereferenced: every call below is refused first
    names = ('n', 'p', 'nrm', 'seed', 'n_hyp', 'thr', 'cos', 'area', 'min_inl', 'best', 'inl', 'work', 'stream')
    ransac = lambda **kw: lib.d3r_plane_ransac(*[dict(dict(n=4, p=one, nrm=None, seed=0, n_hyp=16, thr=0.1, cos=0.0, area=0.01, min_inl=3, best=one,      # noqa: E731
                                                           inl=one, work=one, stream=None), **kw)[a] for a in names])
    for kw in (dict(n=2), dict(p=None), dict(n_hyp=0), dict(n_hyp=2 ** 23 + 1), dict(thr=0.0), dict(thr=-1.0), dict(thr=float('nan')),
               dict(thr=float('inf')), dict(cos=float('nan')), dict(area=0.0), dict(area=-1.0), dict(area=float('nan')), dict(min_inl=2),
               dict(best=None), dict(inl=None), dict(work=None), dict(nrm=one, cos=float('nan'))):
        assert ransac(**kw) == -1, kw
    plane, centre = (C.c_float * 4)(0, 1, 0, -0.5), (C.c_float * 3)(0, 0, 0)
    names = ('n', 'p', 'nrm', 'plane', 'thr', 'cos', 'centre', 'mask', 'count', 'sums', 'work', 'stream')
    support = lambda **kw: lib.d3r_plane_support(*[dict(dict(n=4, p=one, nrm=None, plane=plane, thr=0.1, cos=0.0, centre=centre, mask=None, count=one,      # noqa: E731
                                                             sums=one, work=one, stream=None), **kw)[a] for a in names])
    for kw in (dict(n=0), dict(p=None), dict(plane=None), dict(centre=None), dict(count=None), dict(sums=None), dict(work=None), dict(thr=0.0),
               dict(thr=float('nan')), dict(thr=float('inf')), dict(cos=float('nan')), dict(plane=(C.c_float * 4)(0, 1, 0, float('inf'))),
               dict(plane=(C.c_float * 4)(float('nan'), 1, 0, 0)), dict(centre=(C.c_float * 3)(0, float('nan'), 0))):
        assert support(**kw) == -1, kw


def test_the_build_lists_the_file_and_its_kernels_use_no_scratch():
    import os
    import re
    from dust3r_amd import build
    assert 'cloud_planes.hip' in build.SOURCES and build.EXTRA_FLAGS['cloud_planes.hip'] == build.EXTRA_FLAGS['cloud_features.hip']
    report = os.path.join(build.CSRC, 'cloud_planes.resources.txt')
    text = open(report).read()
    names = re.findall(r'Function Name: (\S+)', text)
    for kernel in ('plane_hyp_kernel', 'plane_score_kernelILb0', 'plane_score_kernelILb1', 'plane_select_kernel', 'plane_mask_kernel', 'plane_support_kernel',
                   'cloud_sums_final_kernelILi9ELi1'):
        assert any(kernel in n for n in names), kernel
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', text)
    assert len(scratch) == len(names) and set(scratch) == {'0'}


# ---- 5. the cloud and its files ---------------------------------------------------------------------------------------------------------------
def _cloud(with_planes=True):
    from dust3r_amd.viz import FusedCloud
    labels = np.where(KIND == 2, -1, KIND).astype(np.int32)
    planes = np.array([[0, 1.0, 0, -0.5], [1.0, 0, 0, -2.5]])
    bounds = (PLANTED.min(axis=0), PLANTED.max(axis=0))
    cloud = FusedCloud(PLANTED, np.full((599, 3), 100, np.uint8), np.ones(599, F32), np.ones(599, np.int32), 0.125, bounds)
    return cloud.with_planes(planes, np.array([300, 168], np.int32), labels) if with_planes else cloud


def test_the_cloud_carries_planes_through_its_host_methods(tmp_path):
    import torch
    from dust3r_amd.export import read_ply
    from dust3r_amd.viz import LABEL_NOISE_COLOR, LABEL_PALETTE, FusedCloud
    cloud = _cloud()
    assert 'plane_labels' in FusedCloud.PER_POINT_ROWS and set(FusedCloud.PER_POINT_ROWS) - set(FusedCloud.PER_POINT) == {'plane_labels'}
    assert cloud.planes.dtype == np.float64 and cloud.planes.shape == (2, 4) and _cloud(False).planes is None
    with pytest.raises(ValueError):
        cloud.with_planes(cloud.planes, cloud.plane_sizes, cloud.plane_labels[:5])
    same = cloud._with(colors=cloud.colors)                                             # a derived cloud keeps the three plane fields
    assert same.planes is cloud.planes and same.plane_sizes is cloud.plane_sizes and same.plane_labels is cloud.plane_labels
    keep = torch.from_numpy(PLANTED[:, 2] < 1.0)
    sub, mask = cloud._subset(keep)
    assert np.array_equal(sub.plane_labels, cloud.plane_labels[mask]) and sub.planes is cloud.planes and sub.plane_sizes is cloud.plane_sizes
    rest, kept = cloud.remove_planes()
    assert np.array_equal(kept, KIND == 2) and len(rest) == 131 and (rest.plane_labels == -1).all()
    no_floor, kept = cloud.remove_planes(labels=[0])
    assert np.array_equal(kept, KIND != 0) and set(no_floor.plane_labels.tolist()) == {-1, 1} and len(no_floor.planes) == 2
    with pytest.raises(ValueError):
        cloud.remove_planes(labels=[2])
    coloured = cloud.colored_by_plane()
    assert (coloured.colors[KIND == 0] == LABEL_PALETTE[0]).all() and (coloured.colors[KIND == 2] == LABEL_NOISE_COLOR).all()
    bare = _cloud(False)
    for call in (bare.remove_planes, bare.colored_by_plane, lambda: bare.upright(cam_centres=[[0, 1, 0]])):
        with pytest.raises(ValueError, match='detect_planes'):
            call()
    with pytest.raises(ValueError):
        cloud.upright()
    with pytest.raises(ValueError, match='one side'):
        cloud.upright(cam_centres=[[1, 0.4, 1], [3, 0.6, 1]])                          # one camera under the floor, on both sides of the wall
    with pytest.raises(ValueError, match='voxel size'):
        FusedCloud(PLANTED, cloud.colors, cloud.weight, cloud.count, float('nan'), cloud.bounds).detect_planes()
    ply = read_ply(cloud.save_ply(str(tmp_path / 'p.ply')))
    assert ply['plane'].dtype == np.int32 and np.array_equal(ply['plane'], cloud.plane_labels) and 'label' not in ply


def test_ply_round_trip_of_the_plane_property_and_unchanged_bytes_without_it(tmp_path):
    from dust3r_amd.export import read_ply, write_ply
    pos = PLANTED[:5]
    col = np.arange(15, dtype=np.uint8).reshape(5, 3)
    w, c = np.arange(5, dtype=F32), np.arange(5, dtype=np.int32) + 1
    lab, pl = np.array([0, -1, 2, 2, 1], np.int32), np.array([-1, 0, 0, 1, -1], np.int64)
    full = read_ply(write_ply(str(tmp_path / 'a.ply'), pos, col, w, c, normals=pos, labels=lab, planes=pl))
    assert np.array_equal(full['plane'], pl) and full['plane'].dtype == np.int32 and np.array_equal(full['label'], lab)
    assert np.array_equal(full['positions'], pos) and np.array_equal(full['normals'], pos) and np.array_equal(full['count'], c)
    only = read_ply(write_ply(str(tmp_path / 'b.ply'), pos, col, planes=pl))
    assert np.array_equal(only['plane'], pl) and set(only) == {'positions', 'colors', 'plane'}
    assert open(str(tmp_path / 'b.ply'), 'rb').read().split(b'end_header')[0].endswith(b'property uchar blue\nproperty int plane\n')
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / 'c.ply'), pos, col, planes=pl.astype(F32))
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / 'c.ply'), pos, col, planes=pl[:4])
    # without planes: the bytes of the file as it has always been written, spelled out here
    rows = np.empty(5, np.dtype([('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('confidence', '<f4'),
                                 ('count', '<i4'), ('label', '<i4')]))
    rows['x'], rows['y'], rows['z'] = pos.T
    rows['red'], rows['green'], rows['blue'] = col.T
    rows['confidence'], rows['count'], rows['label'] = w, c, lab
    header = ('ply\nformat binary_little_endian 1.0\ncomment dust3r_amd fused cloud\nelement vertex 5\nproperty float x\nproperty float y\n'
              'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty float confidence\nproperty int count\n'
              'property int label\nend_header\n')
    for kw in (dict(), dict(planes=None)):
        write_ply(str(tmp_path / 'd.ply'), pos, col, w, c, labels=lab, **kw)
        assert open(str(tmp_path / 'd.ply'), 'rb').read() == header.encode('ascii') + rows.tobytes()


def test_command_line_arguments():
    from dust3r_amd.demo import get_args_parser, wants_fuse
    p = get_args_parser()
    a = p.parse_args(['pics', '--weights', 'w.pth'])
    assert a.fuse_planes is None and not a.fuse_upright and not wants_fuse(a)
    a = p.parse_args(['pics', '--weights', 'w.pth', '--fuse_planes'])
    assert a.fuse_planes == 6 and wants_fuse(a)
    a = p.parse_args(['pics', '--weights', 'w.pth', '--fuse_planes', '3', '--fuse_upright'])
    assert a.fuse_planes == 3 and a.fuse_upright and wants_fuse(a)
    assert wants_fuse(p.parse_args(['pics', '--weights', 'w.pth', '--fuse_upright']))
