"""Plane detection on the GPU: csrc/cloud_planes.hip (cloud_metrics.plane_ransac / plane_support / segment_plane / detect_planes,
FusedCloud.detect_planes / upright, scene.fuse(planes=...)) against the restatement of tests/test_cloud_planes_cpu.py.

What is compared how:
  * d3r_plane_ransac: EXACTLY. h, the count, the number of valid hypotheses and the mask are integers; the plane's four fp64 entries are
    IEEE operations in a stated order on both sides, so they are bit-equal (compared as bytes).
  * d3r_plane_support: the mask and the count exactly; each sum against math.fsum of the same terms, the correctly rounded sum: a sum in
    any order lies within (n - 1) 2^-53 sum |term| of the exact one, so the kernel's within that plus the half ulp of fsum's rounding; the
    header documents the looser 2 (n - 1) 2^-53 sum |term| between two orders, which is what `sum_bound` uses.
  * segment_plane / detect_planes: masks, counts, labels and sizes exactly -- after asserting, on the CPU, that no point lies within 1e-5
    of |e| = thr for any plane of the restatement whose mask is taken, so the last bits of an eigenvector cannot move a point across the
    gate. The refit planes to `model_bound`: the sums' bound carried through the covariance and divided by the eigengap (Davis-Kahan).
No speed is asserted anywhere."""
import math

import numpy as np
import pytest
import torch

from test_cloud_planes_cpu import (KIND, MIN_AREA2, PLANTED, THR, gate_margin, restated_detect, restated_plane_hypotheses,
                                   restated_plane_ransac, restated_residual, restated_segment, restated_support)

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -53
SCHUNK = 2048                       # the points of a scoring workgroup (csrc/cloud_planes.hip)


def _ransac(P, seed, n_hyp, thr, normals=None, cos_min=None, min_area2=None, min_inliers=3):
    from dust3r_amd.cloud_metrics import plane_ransac
    best, inliers = plane_ransac(P, thr, n_hyp, normals, cos_min, min_area2, min_inliers, seed)
    return best.cpu().numpy(), inliers.cpu().numpy()


def _same_ransac(got, want):
    best, inliers = got
    assert best.dtype == np.float64 and best.shape == (7,) and inliers.dtype == np.uint8
    assert (best[0], best[1], best[2]) == (want['h'], want['count'], want['n_valid'])
    assert best[3:].tobytes() == np.asarray(want['model'], np.float64).tobytes()
    assert np.array_equal(inliers.astype(bool), want['inliers']) and set(np.unique(inliers).tolist()) <= {0, 1}


def tiled(n):
    """the planted scene repeated at offsets of 4 along x and z (lattice offsets: every copy's floor stays on y = 0.5), the first n points"""
    copies = -(-n // len(PLANTED))
    parts = [PLANTED + np.array([4.0 * (c % 4), 0.0, 4.0 * (c // 4)], F32) for c in range(copies)]
    return np.concatenate(parts)[:n]


# ---- 1. hypotheses and RANSAC ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_hyp', [1, 255, 256, 257, 513])
def test_ransac_is_the_restatement_on_the_planted_scene(gpu, n_hyp):
    want = restated_plane_ransac(PLANTED, 0, n_hyp, THR, min_area2=MIN_AREA2)
    got = _ransac(torch.from_numpy(PLANTED).to(gpu), 0, n_hyp, THR, min_area2=MIN_AREA2)
    _same_ransac(got, want)
    again = _ransac(PLANTED, 0, n_hyp, THR, min_area2=MIN_AREA2)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()      # the same seed: the same bytes
    if n_hyp > 1:
        assert want['h'] == 32 and want['count'] == 302 and (want['counts'] == 302).sum() >= 2    # tied hypotheses: the lowest wins


@pytest.mark.parametrize('n', [4 * SCHUNK - 1, 4 * SCHUNK, 4 * SCHUNK + 1])
def test_ransac_around_a_multiple_of_the_scoring_chunk(gpu, n):
    P = tiled(n)
    want = restated_plane_ransac(P, 5, 300, THR)                                         # the default min_area2 = (8 thr)^2
    assert want['count'] > 3000 and want['inliers'][P[:, 1] == 0.5].all()
    _same_ransac(_ransac(P, 5, 300, THR), want)


def test_ransac_with_non_finite_points_among_the_samples(gpu):
    rng = np.random.default_rng(7)
    P = PLANTED.copy()
    bad = rng.permutation(len(P))[:200]
    P[bad[:100], rng.integers(0, 3, 100)] = np.nan
    P[bad[100:], rng.integers(0, 3, 100)] = np.inf * rng.choice([-1, 1], 100)
    planes, valid = restated_plane_hypotheses(P, 1, 257, MIN_AREA2)
    assert 0 < valid.sum() < 200                                                         # most samples hold a non-finite point
    want = restated_plane_ransac(P, 1, 257, THR, min_area2=MIN_AREA2)
    assert want['h'] >= 0 and not want['inliers'][bad].any()
    _same_ransac(_ransac(P, 1, 257, THR, min_area2=MIN_AREA2), want)


def degenerate(n, extra):
    """n points of a line on the lattice, every third one a duplicate of its predecessor, and `extra` points off the line"""
    t = np.arange(n) - (np.arange(n) % 3 == 2)
    P = np.stack([0.125 * t, 0.25 * t, np.full(n, 1.0)], axis=1)
    off = np.array([[1.0, 0.0, 3.0], [-2.0, 5.0, 0.5], [0.5, 0.5, -4.0]])[:extra]
    return np.concatenate([P, off]).astype(F32)


def test_duplicate_and_collinear_points_give_invalid_hypotheses_and_whole_invalid_rounds(gpu):
    P = degenerate(999, 1)
    seed = next(s for s in range(64) if len(set(restated_plane_hypotheses(P, s, 1024, MIN_AREA2)[1].reshape(4, 256).any(axis=1).tolist())) == 2)
    _, valid = restated_plane_hypotheses(P, seed, 1024, MIN_AREA2)
    per_round = valid.reshape(4, 256).any(axis=1)
    assert per_round.any() and not per_round.all()                                       # a round with a valid hypothesis and one without
    want = restated_plane_ransac(P, seed, 1024, THR, min_area2=MIN_AREA2)
    assert want['h'] >= 0 and want['inliers'][-1]
    _same_ransac(_ransac(P, seed, 1024, THR, min_area2=MIN_AREA2), want)
    line = degenerate(600, 0)                                                            # nothing but the line: no valid hypothesis at all
    want = restated_plane_ransac(line, 0, 513, THR, min_area2=MIN_AREA2)
    assert want['h'] == -1 and want['n_valid'] == 0
    best, inliers = _ransac(line, 0, 513, THR, min_area2=MIN_AREA2)
    assert best.tolist() == [-1, 0, 0, 0, 0, 0, 0] and not inliers.any()


def test_three_points(gpu):
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], F32)
    want = restated_plane_ransac(P, 0, 4, THR, min_area2=MIN_AREA2)
    assert want['h'] == 0 and want['count'] == 3 and want['n_valid'] == 4 and np.array_equal(np.abs(want['model']), [0, 1, 0, 0])
    _same_ransac(_ransac(P, 0, 4, THR, min_area2=MIN_AREA2), want)
    best, inliers = _ransac(P, 0, 4, THR, min_area2=1.5)                                    # twice the area is 1
    assert best.tolist() == [-1, 0, 0, 0, 0, 0, 0] and not inliers.any()


def test_min_inliers_above_the_best_count(gpu):
    want = restated_plane_ransac(PLANTED, 0, 64, THR, min_area2=MIN_AREA2, min_inliers=303)
    assert want['h'] == -1 and want['n_valid'] == 64
    best, inliers = _ransac(PLANTED, 0, 64, THR, min_area2=MIN_AREA2, min_inliers=303)
    assert best.tolist() == [-1, 0, 64, 0, 0, 0, 0] and inliers.shape == (599,) and not inliers.any()
    _same_ransac(_ransac(PLANTED, 0, 64, THR, min_area2=MIN_AREA2, min_inliers=302), restated_plane_ransac(PLANTED, 0, 64, THR, min_area2=MIN_AREA2,
                                                                                                           min_inliers=302))


def planted_normals():
    """unit normals of the surfaces with either sign, tilted ones on a part of the floor, random ones on the clutter; a zero, a NaN and an
    infinite normal on floor points"""
    rng = np.random.default_rng(3)
    N = rng.standard_normal(PLANTED.shape)
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    floor, wall = np.flatnonzero(KIND == 0), np.flatnonzero(KIND == 1)
    N[floor] = np.array([0, 1.0, 0]) * rng.choice([-1, 1], (len(floor), 1))
    N[wall] = np.array([1.0, 0, 0]) * rng.choice([-1, 1], (len(wall), 1))
    N[floor[:40]] = (0.6, 0.8, 0)                                                       # cos = 0.8 with the floor
    N = N.astype(F32)
    N[floor[40]] = 0
    N[floor[41]] = (np.nan, 1, 0)
    N[floor[42]] = (0, np.inf, 0)
    return N, floor


@pytest.mark.parametrize('cos_min', [0.9, 0.5, 0.0, -1.0])
def test_ransac_with_normals(gpu, cos_min):
    N, floor = planted_normals()
    want = restated_plane_ransac(PLANTED, 2, 257, THR, N, cos_min, MIN_AREA2)
    assert not want['inliers'][floor[40:43]].any() and want['inliers'][floor[43:]].all()
    assert want['inliers'][floor[:40]].all() == (cos_min < 0.8)
    _same_ransac(_ransac(PLANTED, 2, 257, THR, N, cos_min, MIN_AREA2), want)
    dev = _ransac(torch.from_numpy(PLANTED).to(gpu), 2, 257, THR, torch.from_numpy(N).to(gpu), cos_min, MIN_AREA2)
    _same_ransac(dev, want)


@pytest.mark.parametrize('seed', [0, 1])
def test_points_exactly_on_the_gate_are_inliers(gpu, seed):
    """the two lattice surfaces without the clutter, thr = 0.125: the winner is the floor, e is exact, and the wall's first row (y = 0.625)
    lies at e = thr exactly"""
    L, kind = PLANTED[KIND != 2], KIND[KIND != 2]
    want = restated_plane_ransac(L, seed, 257, 0.125, min_area2=MIN_AREA2)
    assert np.array_equal(np.abs(want['model']), [0, 1, 0, 0.5]) and want['count'] == 312 and (want['counts'] == 312).sum() >= 2
    on_gate = np.abs(restated_residual(want['model'].astype(F32), L)) == F32(0.125)
    assert on_gate.sum() == 12 and want['inliers'][on_gate].all() and np.array_equal(on_gate, (kind == 1) & (L[:, 1] == 0.625))
    assert not want['inliers'][(kind == 1) & (L[:, 1] == 0.75)].any()
    _same_ransac(_ransac(L, seed, 257, 0.125, min_area2=MIN_AREA2), want)
    mask, count, _, _ = restated_support(L, want['model'], 0.125, [0, 0.5, 0])
    got_count, _, got_mask = _support(L, want['model'], 0.125, [0, 0.5, 0])
    assert got_count == count == 312 and np.array_equal(got_mask.astype(bool), mask) and mask[on_gate].all()


# ---- 2. the support ---------------------------------------------------------------------------------------------------------------------------
def sum_bound(n, mags, sums):
    """how far a fixed-order fp64 sum of n terms may lie from math.fsum of them: the header's 2 (n - 1) 2^-53 sum |term|, and fsum's rounding"""
    return 2.0 * max(n - 1, 1) * U * mags + U * np.abs(sums)


def _support(P, plane, thr, centre, normals=None, cos_min=None):
    from dust3r_amd.cloud_metrics import plane_support
    count, sums, mask = plane_support(P, plane, thr, centre, normals, cos_min)
    return int(count.cpu()), sums.cpu().numpy(), mask.cpu().numpy()


@pytest.mark.parametrize('n', [599, 256 * 1024 + 77])
def test_support_mask_count_and_moments(gpu, n):
    P = tiled(n)                                                                         # the larger cloud: more workgroups than partials
    P[5] = np.nan
    # the small cloud: a tilted plane; the large one spreads over hundreds of units, where only the floors' own plane holds many points
    plane, centre = np.array([0.001, 0.9999, -0.002, -0.5] if n == 599 else [0, 1.0, 0, -0.5]), np.array([1.25, 0.5, 1.0], F32)
    mask, count, sums, mags = restated_support(P, plane, 0.02, centre)
    assert count > n // 3 and not mask[5]
    got_count, got_sums, got_mask = _support(torch.from_numpy(P).to(gpu), plane, 0.02, centre)
    assert got_count == count and np.array_equal(got_mask.astype(bool), mask) and got_mask.dtype == np.uint8
    bound = sum_bound(n, mags, sums)
    assert (np.abs(got_sums - sums) <= bound).all(), (np.abs(got_sums - sums) / bound).max()
    assert _support(P, plane, 0.02, centre)[1].tobytes() == got_sums.tobytes()           # the same bytes on every run
    from dust3r_amd.cloud_metrics import plane_support
    assert plane_support(P, plane, 0.02, centre, want_mask=False)[2] is None


def test_support_with_normals_and_without_inliers(gpu):
    N, floor = planted_normals()
    plane, centre = np.array([0, 1.0, 0, -0.5]), np.array([0, 0.5, 0], F32)
    for cos_min in (0.9, 0.0):
        mask, count, sums, mags = restated_support(PLANTED, plane, THR, centre, N, cos_min)
        got_count, got_sums, got_mask = _support(PLANTED, plane, THR, centre, N, cos_min)
        assert got_count == count and 250 < count < 300 and np.array_equal(got_mask.astype(bool), mask) and not mask[floor[40:43]].any()
        assert (np.abs(got_sums - sums) <= sum_bound(len(PLANTED), mags, sums)).all()
    got_count, got_sums, got_mask = _support(PLANTED, [0, 1.0, 0, 50.0], THR, centre)
    assert got_count == 0 and not got_sums.any() and not got_mask.any()


# ---- 3. segment_plane and detect_planes -------------------------------------------------------------------------------------------------------
def model_bound(rnd, n):
    """(bound on |delta n| (2-norm), bound on |delta d|) between the plane `plane_from_moments` makes of the kernel's sums and the one it
    makes of the restatement's, for the support pass `rnd` of `restated_segment` over n points. The sums differ by at most `sum_bound`;
    mean = s / count and cov = second / count - mean mean^T carry that into a covariance perturbation E (entrywise, then its Frobenius
    norm; the few roundings of forming cov and LAPACK's backward error, 64 ulps of |cov|, are added on both sides); Davis-Kahan: the
    angle t between the two eigenvectors of the smallest eigenvalue has sin t <= 2 |E| / gap, gap = the distance to the next eigenvalue,
    and two unit vectors at angle t <= pi / 2 differ by 2 sin(t / 2) <= sqrt(2) sin t. d = -n . centroid: |delta d| <= |delta n| |centroid| +
    |delta centroid| and the roundings of the product."""
    from dust3r_amd.cloud_metrics import moments_covariance
    count, sums = rnd['count'], rnd['sums']
    ds = sum_bound(n, rnd['mags'], sums)
    mean, cov = moments_covariance(count, sums)
    dmean = ds[:3] / count + U * np.abs(mean)
    tri = lambda v: np.array([[v[3], v[4], v[5]], [v[4], v[6], v[7]], [v[5], v[7], v[8]]])      # noqa: E731
    am = np.abs(mean)
    E = tri(ds) / count + np.outer(am, dmean) + np.outer(dmean, am) + np.outer(dmean, dmean)
    E += 2 * 4 * U * (np.abs(tri(sums)) / count + np.outer(am, am)) + 2 * 64 * U * np.abs(cov)
    evals = np.linalg.eigvalsh(cov)
    gap = evals[1] - evals[0]
    dn = math.sqrt(2.0) * 2.0 * np.linalg.norm(E) / gap
    centroid = np.asarray(rnd['centre'], np.float64) + mean
    dd = dn * np.linalg.norm(centroid) + np.linalg.norm(dmean) + 8 * U * np.linalg.norm(centroid)
    return dn, dd


def _same_segment(got, seg, P):
    """a `Plane` of the device against `restated_segment` over the points P"""
    assert gate_margin(seg, P, seg['thr']) > 1e-5                                  # on the CPU: no point near the gate of any plane
    assert got.count == seg['count'] and got.inliers.dtype == bool and np.array_equal(got.inliers, seg['inliers'])
    if len(seg['rounds']) == 1:
        assert got.model.tobytes() == seg['model'].tobytes()                            # no refit: the RANSAC plane itself
    else:
        dn, dd = model_bound(seg['rounds'][-2], len(P))
        assert dn < 1e-9 and dd < 1e-9                                                  # the bound is a tight one on these scenes
        assert np.linalg.norm(got.model[:3] - seg['model'][:3]) <= dn and abs(got.model[3] - seg['model'][3]) <= dd
    e = np.asarray(P, F32)[got.inliers].astype(np.float64) @ got.model[:3] + got.model[3]
    last = seg['rounds'][-1]                                                            # rms^2 count = n^T A n + 2 k n . s + count k^2, from the sums
    k = abs(float(got.model[:3] @ np.asarray(last['centre'], np.float64)) + got.model[3])
    scale = float(last['mags'][3:].sum() * 2 + 2 * k * last['mags'][:3].sum() + got.count * k * k)
    assert abs(got.rms ** 2 - float(e @ e) / got.count) <= (2.0 * len(P) + 64) * U * scale / got.count


@pytest.mark.parametrize('n_hyp,refine_rounds', [(64, 3), (513, 1), (64, 0)])
def test_segment_plane_on_the_planted_scene(gpu, n_hyp, refine_rounds):
    from dust3r_amd.cloud_metrics import segment_plane
    seg = restated_segment(PLANTED, THR, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=1, refine_rounds=refine_rounds)
    got = segment_plane(PLANTED, THR, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=1, refine_rounds=refine_rounds)
    _same_segment(got, seg, PLANTED)
    assert got.count == 302 and got.inliers[KIND == 0].all()
    dev = segment_plane(torch.from_numpy(PLANTED).to(gpu), THR, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=1, refine_rounds=refine_rounds, to_host=False)
    assert dev.inliers.is_cuda and dev.inliers.dtype == torch.bool and dev.model.tobytes() == got.model.tobytes() and dev.rms == got.rms
    assert segment_plane(PLANTED, THR, n_hyp=n_hyp, min_area2=MIN_AREA2, min_inliers=400) is None
    assert segment_plane(PLANTED[:2], THR) is None


def noisy_scene():
    """the planted surfaces sampled off the lattice with Gaussian noise of thr / 4 along their normals, and the clutter"""
    rng = np.random.default_rng(12)
    thr = 0.02
    floor = np.c_[rng.uniform(0, 2.5, 900), 0.5 + 0.25 * thr * rng.standard_normal(900), rng.uniform(0, 2.0, 900)]
    wall = np.c_[2.5 + 0.25 * thr * rng.standard_normal(500), rng.uniform(0.6, 2.3, 500), rng.uniform(0, 1.5, 500)]
    clutter = rng.uniform(0, 2.5, (200, 3))
    P = np.concatenate([floor, wall, clutter]).astype(F32)
    kind = np.repeat([0, 1, 2], [900, 500, 200])
    order = rng.permutation(len(P))
    return P[order], kind[order], thr


def test_segment_and_detect_on_a_noisy_scene_against_the_restatement(gpu):
    from dust3r_amd.cloud_metrics import detect_planes, segment_plane
    P, kind, thr = noisy_scene()
    seg = restated_segment(P, thr, n_hyp=257, seed=4)
    assert len(seg['rounds']) >= 2 and seg['count'] > 850                                # the refit ran
    _same_segment(segment_plane(P, thr, n_hyp=257, seed=4), seg, P)
    planes, sizes, labels, segments = restated_detect(P, thr, max_planes=4, min_inliers=100, n_hyp=257, seed=4)
    assert len(planes) == 2 and (labels[kind == 0] == 0).mean() > 0.99 and (labels[kind == 1] == 1).mean() > 0.99
    for s, rows in segments:
        assert gate_margin(s, P[rows], thr) > 1e-5
    got = detect_planes(P, thr, max_planes=4, min_inliers=100, n_hyp=257, seed=4)
    assert np.array_equal(got.plane_labels, labels) and np.array_equal(got.plane_sizes, sizes) and got.planes.shape == (2, 4)
    for r, (s, rows) in enumerate(segments):
        dn, dd = model_bound(s['rounds'][-2], len(rows))
        assert np.linalg.norm(got.planes[r, :3] - planes[r, :3]) <= dn < 1e-9 and abs(got.planes[r, 3] - planes[r, 3]) <= dd < 1e-9


@pytest.mark.parametrize('n_hyp', [64, 513])
def test_detect_planes_on_the_planted_scene(gpu, n_hyp):
    from dust3r_amd.cloud_metrics import detect_planes
    planes, sizes, labels, segments = restated_detect(PLANTED, THR, max_planes=6, min_inliers=100, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=3)
    assert sizes.tolist() == [302, 168]
    for s, rows in segments:
        assert gate_margin(s, PLANTED[rows], THR) > 1e-5
    got = detect_planes(PLANTED, THR, max_planes=6, min_inliers=100, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=3)
    assert got.plane_labels.dtype == np.int32 and got.plane_sizes.dtype == np.int32 and got.planes.dtype == np.float64
    assert np.array_equal(got.plane_labels, labels) and np.array_equal(got.plane_sizes, sizes)
    for r, (s, rows) in enumerate(segments):
        if len(s['rounds']) == 1:
            assert got.planes[r].tobytes() == planes[r].tobytes()
        else:
            dn, dd = model_bound(s['rounds'][-2], len(rows))
            assert np.linalg.norm(got.planes[r, :3] - planes[r, :3]) <= dn < 1e-9 and abs(got.planes[r, 3] - planes[r, 3]) <= dd < 1e-9
    one = detect_planes(PLANTED, THR, max_planes=1, min_inliers=100, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=3)
    assert np.array_equal(one.plane_labels, np.where(labels == 0, 0, -1)) and one.plane_sizes.tolist() == [302]
    none = detect_planes(PLANTED, THR, max_planes=0)
    assert none.planes.shape == (0, 4) and (none.plane_labels == -1).all() and len(none.plane_sizes) == 0
    dev = detect_planes(torch.from_numpy(PLANTED).to(gpu), THR, max_planes=6, min_inliers=100, n_hyp=n_hyp, min_area2=MIN_AREA2, seed=3, to_host=False)
    assert dev.plane_labels.is_cuda and dev.plane_sizes.is_cuda and np.array_equal(dev.plane_labels.cpu().numpy(), labels)
    N, floor = planted_normals()
    with_normals = restated_detect(PLANTED, THR, max_planes=2, min_inliers=100, n_hyp=n_hyp, normals=N, cos_min=0.9, min_area2=MIN_AREA2, seed=3)
    got = detect_planes(PLANTED, THR, max_planes=2, min_inliers=100, n_hyp=n_hyp, normals=N, cos_min=0.9, min_area2=MIN_AREA2, seed=3)
    for s, rows in with_normals[3]:
        assert gate_margin(s, PLANTED[rows], THR) > 1e-5
    assert np.array_equal(got.plane_labels, with_normals[2]) and got.plane_sizes.tolist() == with_normals[1].tolist() and (got.plane_labels[floor[:43]] != 0).all()


# ---- 4. through the cloud and the scene -------------------------------------------------------------------------------------------------------
def _planted_cloud(on_device=None):
    from dust3r_amd.viz import FusedCloud
    P = PLANTED if on_device is None else torch.from_numpy(PLANTED).to(on_device)
    wrap = (lambda a: a) if on_device is None else (lambda a: torch.from_numpy(a).to(on_device))
    return FusedCloud(P, wrap(np.full((599, 3), 100, np.uint8)), wrap(np.ones(599, F32)), wrap(np.ones(599, np.int32)), 0.005,
                      (PLANTED.min(axis=0), PLANTED.max(axis=0)))


def test_fused_cloud_detects_removes_and_stands_upright(gpu):
    from dust3r_amd.cloud_metrics import detect_planes, upright_similarity
    cloud = _planted_cloud()
    # thr: 2 voxels = 0.01; without refits the planes are the RANSAC winners, exact on the lattice: (0, +-1, 0, -+0.5) and (+-1, 0, 0, -+2.5)
    found = cloud.detect_planes(max_planes=2, min_inliers=100, min_area2=MIN_AREA2, n_hyp=64, seed=3, refine_rounds=0)
    by_hand = detect_planes(PLANTED, 2 * 0.005, max_planes=2, min_inliers=100, min_area2=MIN_AREA2, n_hyp=64, seed=3, refine_rounds=0)
    assert np.array_equal(np.abs(found.planes), [[0, 1, 0, 0.5], [1, 0, 0, 2.5]])
    assert np.array_equal(found.plane_labels, by_hand.plane_labels) and found.planes.tobytes() == by_hand.planes.tobytes()
    assert found.plane_sizes.tolist() == [302, 168] and found.positions is cloud.positions and isinstance(found.plane_labels, np.ndarray)
    rest, keep = found.remove_planes()
    assert len(rest) == 599 - 470 and np.array_equal(keep, found.plane_labels < 0)
    cams = np.array([[0.5, 1.5, 0.5], [3.0, 1.2, 1.0]])                                   # above the floor, on both sides of the wall
    up, T = found.upright(cam_centres=cams)
    assert np.array_equal(T, upright_similarity(-found.planes[0] if found.planes[0][1] < 0 else found.planes[0]))
    assert np.abs(up.positions[KIND == 0][:, 1]).max() <= 1e-5 and up.tracks is None and np.array_equal(up.plane_labels, found.plane_labels)
    assert np.abs(np.abs(up.planes[0]) - [0, 1, 0, 0]).max() <= 1e-9                          # the planes moved with the points
    assert np.abs(up.positions[KIND == 1] @ up.planes[1][:3].astype(F32) + F32(up.planes[1][3])).max() <= 1e-5
    assert ((cams @ T[:3, :3].T + T[:3, 3])[:, 1] > 0).all()                              # the cameras end above the ground
    dev = _planted_cloud(gpu).detect_planes(max_planes=2, min_inliers=100, min_area2=MIN_AREA2, n_hyp=64, seed=3, refine_rounds=0)
    assert dev.plane_labels.is_cuda and np.array_equal(dev.plane_labels.cpu().numpy(), found.plane_labels)
    rest_dev, keep_dev = dev.remove_planes(labels=[1])
    assert keep_dev.is_cuda and len(rest_dev) == 599 - 168
    assert dev.colored_by_plane().colors.is_cuda


@pytest.fixture(scope='module')
def scene(gpu):
    from test_fuse_gpu import _scene
    return _scene(gpu, 3, 24, 32, 5)


def test_scene_fuse_with_planes_and_upright(gpu, scene):
    """The synthetic scene of the fuse tests has its cameras on a circle AROUND the surfaces they look at (synthetic_scene: radius 2, 120
    degrees apart, each surface a bumpy patch through the origin that faces its camera). No plane through such a patch has all three
    cameras on one side -- the two others stand 1 behind it -- so `ground_plane` rightly finds no ground for the scene's own cameras and
    scene.fuse(planes=2, upright=True) raises the documented ValueError. That the motion puts the ground at height 0 is therefore checked on
    this scene with the cameras that face the largest plane, through FusedCloud.upright(cam_centres=...), which is the call
    scene.fuse(upright=True) makes with all of them."""
    from dust3r_amd.cloud_metrics import ground_plane, upright_similarity
    a, b = scene.fuse(), scene.fuse(planes=None, upright=False)
    assert a.planes is None and a.plane_labels is None
    for name in ('positions', 'colors', 'weight', 'count'):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes()                     # the defaults are untouched
    found = scene.fuse(planes=2)
    by_hand = a.detect_planes(max_planes=2)
    assert len(found) == len(a) and np.array_equal(found.plane_labels, by_hand.plane_labels) and found.planes.tobytes() == by_hand.planes.tobytes()
    assert 1 <= len(found.planes) <= 2 and np.array_equal(np.bincount(found.plane_labels[found.plane_labels >= 0]), found.plane_sizes)
    cleaned, keep = found.remove_outliers()                                              # the labels travel with the points that stay
    assert 0 < keep.sum() < len(found) or keep.all()
    assert np.array_equal(cleaned.plane_labels, found.plane_labels[keep]) and cleaned.planes is found.planes
    chained = scene.fuse(outliers=2.0, planes=dict(max_planes=2, n_hyp=1024), tracks=True)      # planes after the removal, before the tracks
    assert chained.tracks.n_points == len(chained) == len(chained.plane_labels) == len(cleaned)
    assert np.array_equal(chained.positions, cleaned.positions)
    with pytest.raises(ValueError, match='planes'):
        scene.fuse(planes=dict(radius=1.0))
    thr = 2 * found.voxel_size
    cams = scene.get_im_poses().detach().cpu().numpy()[:, :3, 3].astype(np.float64)
    e = cams @ found.planes[0, :3] + found.planes[0, 3]
    assert (e > thr).any() and (e < -thr).any()                                          # cameras on both sides of the largest plane
    assert ground_plane(found.planes, found.plane_sizes, cams, thr) is None
    with pytest.raises(ValueError, match='one side'):
        scene.fuse(planes=2, upright=True)
    facing = cams[e * np.sign(e[np.argmax(np.abs(e))]) > thr]                              # the cameras in front of it
    ground = ground_plane(found.planes, found.plane_sizes, facing, thr)
    assert ground is not None and np.array_equal(np.abs(ground), np.abs(found.planes[0]))
    with_tracks = scene.fuse(planes=2, tracks=True)
    up, T = with_tracks.upright(cam_centres=facing)
    assert with_tracks.tracks is not None and up.tracks is None                          # built before the motion, dropped by it
    assert np.array_equal(T, upright_similarity(ground)) and up.positions.tobytes() == found.transform(T).positions.tobytes()
    assert np.abs(np.abs(up.planes[0]) - [0, 1, 0, 0]).max() <= 1e-9                       # the ground is y = 0 ...
    on_ground = up.positions[up.plane_labels == 0]
    assert len(on_ground) == found.plane_sizes[0] and np.abs(on_ground[:, 1]).max() <= thr * (1 + 1e-3)      # ... and its points lie on it
    assert ((facing @ T[:3, :3].T + T[:3, 3])[:, 1] > thr).all()                           # the cameras that see it stand above it


def test_demo_writer_writes_the_planes_and_the_motion(gpu, scene, tmp_path):
    import copy
    import json
    from dust3r_amd import demo
    from dust3r_amd.export import read_ply
    demo.write_cameras(str(tmp_path), scene)
    written = demo.write_fused(str(tmp_path), copy.deepcopy(scene), min_conf_thr=1.0, planes=2)
    ply = read_ply(written[0])
    doc = json.load(open(str(tmp_path / 'cameras.json')))
    assert doc['planes']['sizes'] == np.bincount(ply['plane'][ply['plane'] >= 0]).tolist() and len(doc['planes']['models']) == len(doc['planes']['sizes'])
    assert 'upright' not in doc and 'clusters' not in doc
    # this scene's cameras surround its surfaces (see the test above): no ground, so the cloud stays as it is and no motion is reported
    written = demo.write_fused(str(tmp_path), copy.deepcopy(scene), min_conf_thr=1.0, upright=True)
    stood = read_ply(written[0])
    doc = json.load(open(str(tmp_path / 'cameras.json')))
    assert 'upright' not in doc and len(doc['planes']['sizes']) >= len(np.unique(ply['plane'][ply['plane'] >= 0]))      # upright implies six planes
    assert np.array_equal(stood['positions'], ply['positions'])
