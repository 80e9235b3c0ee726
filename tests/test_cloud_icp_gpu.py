"""Cloud registration on the GPU: the kernels of csrc/cloud_icp.hip and cloud_metrics.register_clouds against the numpy restatements of
tests/test_cloud_icp_cpu.py. The transform is compared bit for bit, the used mask and the count exactly; every sum within
2 (n - 1) 2^-53 sum |term| of numpy's fp64 sum of the same doubles (only the order of addition differs); a whole registration against the
restated loop by the bar 'no further from the restatement than the restatement is from the truth'."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from test_cloud_icp_cpu import (CASES, RIGID_INIT, STAGES, TRUTH, pca_normals, restated_case, restated_register, restated_transform,
                                restated_used_and_sums, scene, similarity, similarity_distance)
from test_cloud_metrics_cpu import brute_force

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -53


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(a):
    """float32 rows as uint32 with every NaN made one value: the payload of a NaN is not part of the contract"""
    a = np.ascontiguousarray(a, F32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


# ---- 1. the transform ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 70001])
def test_transform_is_bit_equal(gpu, n):
    from dust3r_amd.cloud_metrics import similarity_parts, transform_points
    rng = np.random.default_rng(n)
    P = (rng.standard_normal((n, 3)) * 3).astype(F32)
    N = rng.standard_normal((n, 3)).astype(F32)
    P[::7, 0], P[3::11, 1], P[5::13, 2], N[2::17, 1] = np.nan, np.inf, -np.inf, np.nan
    M, R, _ = similarity_parts(TRUTH)
    want, want_n = restated_transform(P, M, N, R)
    assert not np.isfinite(want[::7]).any() and not np.isfinite(want[3::11]).any() and not np.isfinite(want[5::13]).any()
    got, got_n = transform_points(_dev(P, gpu), TRUTH, normals=_dev(N, gpu))
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)) and np.array_equal(_bits(got_n.cpu().numpy()), _bits(want_n))
    alone, none = transform_points(P, TRUTH)                                           # host array in, no normals
    assert none is None and alone.is_cuda and np.array_equal(_bits(alone.cpu().numpy()), _bits(want))


# ---- 2. the sums ----------------------------------------------------------------------------------------------------------------------------
N_REF, GATE, COS_MIN = 300, F32(0.75), F32(0.6)


def _sums_inputs(n):
    """rows that meet every gate from both sides; the special rows repeat with period 16, so n = 1 holds one of them and n >= 255 all"""
    rng = np.random.default_rng(1000 + n)
    ref = rng.standard_normal((N_REF, 3)).astype(F32)
    ref_n = rng.standard_normal((N_REF, 3))
    ref_n = (ref_n / np.linalg.norm(ref_n, axis=1, keepdims=True)).astype(F32)
    ref[5, 1], ref[6, 0] = np.nan, np.inf
    ref_n[8], ref_n[9, 2] = 0, np.nan
    ref_n[7] = (1, 0, 0)
    moved = (rng.standard_normal((n, 3)) + 0.5).astype(F32)
    idx = rng.integers(10, N_REF, n).astype(np.int32)
    d2 = (rng.random(n) * 0.8).astype(F32) ** 2                                        # most rows inside the gate, a fifth outside
    g2 = GATE * GATE
    i = np.arange(n)
    special = {1: 'idx -1', 2: 'idx n_ref', 3: 'nan point', 4: 'nan ref', 5: 'inf ref', 6: 'zero normal', 7: 'nan normal', 8: 'at gate',
               9: 'above gate', 12: 'idx beyond', 13: 'inf d2'}
    rows_of = lambda k: i[i % 16 == k] if n > 1 else (i if k == 8 else i[:0])      # noqa: E731
    for k, what in special.items():
        rows = rows_of(k)
        if what == 'idx -1':
            idx[rows] = -1
        elif what == 'idx n_ref':
            idx[rows] = N_REF
        elif what == 'idx beyond':
            idx[rows] = 2 ** 31 - 1
        elif what == 'nan point':
            moved[rows, 2] = np.nan
        elif what in ('nan ref', 'inf ref', 'zero normal', 'nan normal'):
            idx[rows] = {'nan ref': 5, 'inf ref': 6, 'zero normal': 8, 'nan normal': 9}[what]
        elif what == 'at gate':
            d2[rows] = g2
        elif what == 'above gate':
            d2[rows] = np.nextafter(g2, F32(np.inf))
        else:
            d2[rows] = np.inf
    # the source normals: near the paired reference normal (cosine about 0.98), turned away in the rows 14 of 16
    near = ref_n[np.clip(idx, 10, N_REF - 1)].astype(np.float64) + 0.1 * rng.standard_normal((n, 3))
    moved_n = (near / np.linalg.norm(near, axis=1, keepdims=True)).astype(F32)
    moved_n[rows_of(14)] *= F32(-1)
    for k, m_x in ((10, COS_MIN), (11, np.nextafter(COS_MIN, F32(-1)))):               # the cosine against the normal (1, 0, 0) is m_x itself
        idx[rows_of(k)], d2[rows_of(k)] = 7, 0.01
        moved_n[rows_of(k)] = (m_x, 0, 0)
    centre = F32([0.25, -0.5, 0.125])
    return moved, moved_n, ref, ref_n, d2, idx, centre


@pytest.mark.parametrize('n', [1, 63, 64, 65, 255, 256, 257, 70001])
@pytest.mark.parametrize('metric', ['point', 'plane'])
def test_sums_against_the_restatement(gpu, metric, n):
    """used and count exact; every sum within 2 (n - 1) 2^-53 sum |term| (n = 1: equal); without a used row the sums are exactly 0; the
    same bytes twice. With and without the cosine gate; the point metric also without any normals."""
    from dust3r_amd.cloud_metrics import icp_sums
    moved, moved_n, ref, ref_n, d2, idx, centre = _sums_inputs(n)
    dev = {k: _dev(v, gpu) for k, v in dict(moved=moved, moved_n=moved_n, ref=ref, ref_n=ref_n, d2=d2, idx=idx).items()}
    for cos_gate, with_ref_normals in ((False, True), (True, True)) + (((False, False),) if metric == 'point' else ()):
        kw = dict(ref_normals=ref_n if with_ref_normals else None, moved_normals=moved_n if cos_gate else None, cos_min=COS_MIN if cos_gate else None)
        used, count, sums, terms = restated_used_and_sums(moved, ref, d2, idx, metric, GATE, centre, **kw)
        run = lambda: icp_sums(dev['moved'], dev['ref'], dev['d2'], dev['idx'], metric, GATE, centre, ref_normals=dev['ref_n'] if with_ref_normals else None,      # noqa: E731
                               moved_normals=dev['moved_n'] if cos_gate else None, cos_min=kw['cos_min'], want_used=True)
        got_count, got_sums, got_used = run()
        if n >= 255:
            i = np.arange(n)
            assert used[i % 16 == 8].all() and not used[i % 16 == 9].any() and 0.2 * n < count < 0.6 * n
            assert used[i % 16 == 10].all() and used[i % 16 == 11].any() != cos_gate and used[i % 16 == 14].any() != cos_gate
            assert not used[np.isin(i % 16, [1, 2, 3, 4, 5, 12, 13])].any() and (used[np.isin(i % 16, [6, 7])].any() == (metric == 'point' and not cos_gate))
        assert np.array_equal(got_used.cpu().numpy().astype(bool), used) and int(got_count) == count
        bound = 2 * (n - 1) * U * np.abs(terms).sum(axis=0)
        err = np.abs(got_sums.cpu().numpy() - sums)
        assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
        again = run()
        assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(again, (got_count, got_sums, got_used)))
    none = icp_sums(dev['moved'], dev['ref'], dev['d2'], torch.full_like(dev['idx'], -1), metric, GATE, centre, ref_normals=dev['ref_n'], want_used=True)
    assert int(none[0]) == 0 and not none[1].cpu().numpy().any() and not none[2].any() and len(none[1]) == (18 if metric == 'point' else 36)


# ---- 3. one iteration and whole registrations on the scene of the CPU file ------------------------------------------------------------------
def _cloud(positions, normals, gpu):
    """a reference cloud that brings its own normals, on the device"""
    from dust3r_amd.viz import FusedCloud
    P = _dev(positions, gpu)
    return FusedCloud(P, None, None, None, voxel_size=float('nan'), bounds=(positions.min(axis=0), positions.max(axis=0)), normals=_dev(normals, gpu))


def _bounds_centre(dst):
    return ((dst.min(axis=0).astype(np.float64) + dst.max(axis=0).astype(np.float64)) * 0.5).astype(F32)


@pytest.mark.parametrize('metric', ['point', 'plane'])
def test_one_iteration_at_a_given_similarity(gpu, metric):
    """At S = 3 degrees and 3 % from the truth, gate 0.1: the neighbours are the brute force's, the used set the restatement's, and the
    update agrees to what the bound on the sums allows. Plane: H x = -g with |dH|, |dg| <= the sums' bounds gives
    |dx| <= |H^-1| (|dg| + |dH| |x|) / (1 - |H^-1| |dH|) (2-norms; Frobenius for the bounds), plus the solve's own rounding
    cond(H) 2^-52 |x| on either side; an entry of delta moves by at most (1 + |c|) e^sigma |dx| to first order, doubled here. Point: the
    rotation is the polar factor of the covariance C, |dR|_F <= 2 |dC|_F / (s_2 + s_3) (Li 1995), dC from the bounds on the moments."""
    from dust3r_amd.cloud_metrics import icp_sums, icp_update, nearest_in_cloud, plane_system, transform_points
    src, dst, normals = scene('fresh')
    S = similarity((3, -1, 2), 3.0, 1.03, (0.01, 0.02, -0.01)) @ TRUTH
    gate, c = 0.1, _bounds_centre(dst)
    moved = restated_transform(src, S[:3, :4].astype(F32).reshape(12))
    d2, idx = brute_force(moved, dst, gate)
    used, count, sums, terms = restated_used_and_sums(moved, dst, d2, idx, metric, gate, c, ref_normals=normals)
    assert 2000 < count < len(src)                                                     # the gate drops the far outliers
    moved_d, _ = transform_points(_dev(src, gpu), S)
    d2_d, idx_d = nearest_in_cloud(moved_d, _dev(dst, gpu), gate, to_host=False)
    assert np.array_equal(moved_d.cpu().numpy(), moved) and np.array_equal(idx_d.cpu().numpy(), idx) and np.array_equal(d2_d.cpu().numpy(), d2)
    got_count, got_sums, got_used = icp_sums(moved_d, _dev(dst, gpu), d2_d, idx_d, metric, gate, c, ref_normals=_dev(normals, gpu), want_used=True)
    assert np.array_equal(got_used.cpu().numpy().astype(bool), used) and int(got_count) == count
    got_sums = got_sums.cpu().numpy()
    bound = 2 * (len(src) - 1) * U * np.abs(terms).sum(axis=0)
    assert (np.abs(got_sums - sums) <= bound).all()
    want, rmse, _ = icp_update(metric, sums, count, c.astype(np.float64))
    got, got_rmse, reason = icp_update(metric, got_sums, count, c.astype(np.float64))
    assert reason is None and abs(got_rmse - rmse) <= bound[-1] / (2 * count * rmse) * 2
    if metric == 'plane':
        H, g, _ = plane_system(sums)
        dH, dg, _ = plane_system(bound)
        x = np.linalg.solve(H, -g)
        inv = np.linalg.norm(np.linalg.inv(H), 2)
        dx = inv * (np.linalg.norm(dg) + np.linalg.norm(dH) * np.linalg.norm(x)) / (1 - inv * np.linalg.norm(dH)) + 2 * np.linalg.cond(H) * 2 * U * np.linalg.norm(x)
        allowed = 2 * (1 + np.linalg.norm(c)) * math.exp(x[6]) * dx
    else:
        n, m = sums[0], sums
        mx, my = m[1:4] / n, m[4:7] / n
        C = (m[7:16].reshape(3, 3) / n).T - np.outer(my, mx)
        dC = bound[7:16].reshape(3, 3).T / n + (np.outer(bound[4:7], np.abs(mx)) + np.outer(np.abs(my), bound[1:4])) / n
        sv = np.linalg.svd(C, compute_uv=False)
        dR = 2 * np.linalg.norm(dC) / (sv[1] + sv[2]) + 64 * U                          # and the rounding of the SVD's own products
        got, want = got[:3, :3] / np.cbrt(np.linalg.det(got[:3, :3])), want[:3, :3] / np.cbrt(np.linalg.det(want[:3, :3]))
        allowed = dR
    print(f'{metric}: delta differs by {np.abs(got - want).max():.3e}, allowed {allowed:.3e}')
    assert np.abs(got - want).max() <= allowed


def _register(gpu, kind, metric, with_scale, **kw):
    from dust3r_amd.cloud_metrics import register_clouds
    src, dst, normals = scene(kind)
    return register_clouds(_dev(src, gpu), _cloud(dst, normals, gpu), STAGES, init=None if with_scale else RIGID_INIT, with_scale=with_scale,
                           metric=metric, **kw)


def assert_end_to_end_bar(S, n_pairs, restated, what, rigid=False):
    """S no further from the restatement's than the restatement's is from the truth: angle, relative scale, translation. A rigid run does
    not estimate the scale: both sides carry 1.08 through some twenty fp64 products and one cube root of a determinant, and the
    restatement sits within an ulp of it, so there the scale's bar is 64 2^-53, the rounding of those products."""
    S_r, history, _ = restated
    bar, got = similarity_distance(S_r, TRUTH), similarity_distance(S, S_r)
    print(f'{what}: from the restatement {got[0]:.3g} deg, scale {got[1]:.3g}, translation {got[2]:.3g}; the restatement from the truth '
          f'{bar[0]:.3g} deg, {bar[1]:.3g}, {bar[2]:.3g}; pairs {n_pairs} / {history[-1][1]}')
    assert got[0] <= bar[0] and got[1] <= (max(bar[1], 64 * U) if rigid else bar[1]) and got[2] <= bar[2]
    assert abs(n_pairs - history[-1][1]) <= 0.01 * history[-1][1]


@pytest.mark.parametrize('kind,metric,with_scale', [('fresh', 'plane', True), ('fresh', 'plane', False), ('subset', 'point', True)])
def test_end_to_end_against_the_restatement(gpu, kind, metric, with_scale):
    reg = _register(gpu, kind, metric, with_scale)
    assert reg.converged and reg.reason == 'converged' and reg.iterations == len(reg.history) and reg.n_valid == 5250
    assert reg.history[-1] == (len(STAGES) - 1, reg.n_pairs, reg.rmse) and reg.scale == pytest.approx(np.cbrt(np.linalg.det(reg.similarity[:3, :3])))
    assert_end_to_end_bar(reg.similarity, reg.n_pairs, restated_case(kind, metric, with_scale), f'{kind} {metric} with_scale={with_scale}', rigid=not with_scale)


def test_kept_grids_give_the_bytes_of_rebuilt_grids(gpu):
    kept, rebuilt = _register(gpu, 'fresh', 'plane', True), _register(gpu, 'fresh', 'plane', True, _rebuild_grids=True)
    assert kept.similarity.tobytes() == rebuilt.similarity.tobytes() and kept.history == rebuilt.history and kept.iterations > 6


def test_register_clouds_edge_cases(gpu):
    """no pair at the first iteration raises; its own PCA normals (k = 16) serve when the reference has none; the cosine gate needs normals
    on both sides; a reference on one plane ends with a reason"""
    from dust3r_amd.cloud_metrics import register_clouds
    src, dst, normals = scene('subset')
    with pytest.raises(ValueError, match='no source point has a neighbour'):
        register_clouds(src + F32(50), dst, 0.1)
    with pytest.raises(ValueError, match='cos_min needs normals'):
        register_clouds(src, dst, 0.3, cos_min=0.5)
    own = register_clouds(src, dst, STAGES)                                            # host arrays, normals computed on the device
    ang, ds, dt = similarity_distance(own.similarity, TRUTH)
    print(f'own normals: {ang:.3g} deg, scale {ds:.3g}, translation {dt:.3g} from the truth')
    assert own.converged and ang <= 0.022 and ds <= 2e-5 and dt <= 4.6e-5              # the subset case's bar of the restatement
    rng = np.random.default_rng(9)
    flat = np.concatenate([rng.random((2000, 2)), np.zeros((2000, 1))], axis=1).astype(F32)
    up = np.tile(F32([[0, 0, 1]]), (len(flat), 1))
    reg = register_clouds(flat[:500] + F32([0, 0, 0.01]), _cloud(flat, up, gpu), 0.1)
    assert not reg.converged and 'singular' in reg.reason and reg.iterations == 1 and np.array_equal(reg.similarity, np.eye(4))


def test_fused_cloud_transform(gpu):
    from dust3r_amd.cloud_metrics import similarity_parts
    from dust3r_amd.viz import FusedCloud
    rng = np.random.default_rng(4)
    P, N = rng.standard_normal((1000, 3)).astype(F32), rng.standard_normal((1000, 3)).astype(F32)
    colors, weight, count = rng.integers(0, 255, (1000, 3)).astype(np.uint8), rng.random(1000).astype(F32), rng.integers(1, 9, 1000).astype(np.int32)
    cloud = FusedCloud(P, colors, weight, count, voxel_size=0.25, bounds=(P.min(axis=0), P.max(axis=0)), normals=N, curvature=weight)
    M, R, s = similarity_parts(TRUTH)
    want, want_n = restated_transform(P, M, N, R)
    for c in (cloud, FusedCloud(_dev(P, gpu), _dev(colors, gpu), _dev(weight, gpu), _dev(count, gpu), voxel_size=0.25, bounds=cloud.bounds, normals=_dev(N, gpu))):
        out = c.transform(TRUTH)
        assert type(out.positions) is type(c.positions) and out.colors is c.colors and out.weight is c.weight and out.count is c.count
        host = lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t         # noqa: E731
        assert np.array_equal(host(out.positions), want) and np.array_equal(host(out.normals), want_n) and out.voxel_size == pytest.approx(0.25 * s)
        assert np.array_equal(out.bounds[0], want.min(axis=0)) and np.array_equal(out.bounds[1], want.max(axis=0)) and out.curvature is c.curvature
    assert np.array_equal(cloud.positions, P)                                          # the cloud itself is not moved


# ---- 4. evaluate_scene(refine='icp') --------------------------------------------------------------------------------------------------------
N_VIEWS, H, W = 4, 24, 32


@pytest.fixture(scope='module')
def scene_and_gt(gpu):
    """the scene of tests/test_cloud_metrics_gpu.py: synthetic_scene(4 views, 24 x 32, perturb=False) in an aligner; it IS the ground truth
    in a scaled world"""
    from dust3r_amd.cloud_opt import global_aligner
    from dust3r_amd.synthetic import outdoor_scene, synthetic_scene
    out, init, gt = synthetic_scene(N_VIEWS, H, W, seed=1, scene_graph='complete', symmetrize=True, noise=0.002, device=gpu, perturb=False)
    aligned = global_aligner(out, device=gpu, verbose=False)
    aligned.load_state_dict(init)
    aligned.imgs = [outdoor_scene(H, W, seed=k).astype(np.float32) / 255 for k in range(N_VIEWS)]
    aligned.min_conf_thr = float(aligned._im_conf[:, :H * W].median())
    c2w, f, depth = gt['cam2world'].numpy().astype(np.float64), float(gt['focal']), gt['depth'].numpy().astype(np.float64)
    vs, us = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    rays = np.stack(((us - W / 2) / f, (vs - H / 2) / f, np.ones_like(us)), axis=-1)
    rng = np.random.default_rng(3)
    views = []
    for k in range(N_VIEWS):
        pts = (depth[k][..., None] * rays) @ c2w[k, :3, :3].T + c2w[k, :3, 3]
        views.append(dict(pts3d=pts.astype(np.float32), valid_mask=rng.random((H, W)) < 0.9, camera_pose=c2w[k].astype(np.float32)))
    return aligned, views


def _report(m, what):
    print(f"{what}: ate_rmse {m['ate_rmse']:.3e}, rotation mean {m['rot_err_mean_deg']:.3e} max {m['rot_err_max_deg']:.3e} deg, fscore {m['fscore']}, "
          f"accuracy {m['accuracy']:.3e}, completeness {m['completeness']:.3e}")


def test_evaluate_scene_refine(gpu, scene_and_gt):
    """refine=None is today's dict. refine='icp' after the points alignment is not worse in the pose errors and the F-score: this scene IS
    the ground truth to fp32 rounding (ate_rmse 3e-7), ICP between two differently sampled clouds ends 0.03 degrees off and raises
    `overall`, so the refinement is not accepted (details['refined'] is False) and the first alignment is reported. After an alignment
    turned by 2 degrees about the ground truth's middle it is accepted and strictly better in the pose errors and the F-score. The
    thresholds: the turn displaces a point at distance d from the middle by 0.035 d, at most 0.7 voxels in this scene of radius 1 and
    voxel 0.051; at a threshold of a voxel or more a displaced point still finds a neighbour and the F-score cannot tell the alignments
    apart (and is 1 on both sides from 4 voxels on), so the F-score is taken at 1/8, 1/4 and 1/2 voxel."""
    from dust3r_amd.evaluation import evaluate_scene
    aligned, views = scene_and_gt
    plain, det = evaluate_scene(aligned, views, return_details=True)
    assert evaluate_scene(aligned, views, refine=None) == plain and 'registration' not in det and 'refined' not in det
    v = plain['voxel_size']
    th = [v / 8, v / 4, v / 2]
    plain = evaluate_scene(aligned, views, thresholds=th)
    assert evaluate_scene(aligned, views, align=det['similarity'], thresholds=th) == plain      # a given similarity takes the computed one's place
    refined, rdet = evaluate_scene(aligned, views, thresholds=th, refine='icp', return_details=True)
    _report(plain, 'refine=None'), _report(refined, "refine='icp'")
    reg = rdet['registration']
    print(f'registration: {reg.iterations} iterations, {reg.reason}, rmse {reg.rmse:.3e}, accepted {rdet["refined"]}')
    assert reg.iterations >= 1 and rdet['refined'] in (True, False) and set(refined) == set(plain) and refined['voxel_size'] == v
    want = reg.similarity @ det['similarity'] if rdet['refined'] else det['similarity']
    assert np.allclose(rdet['similarity'], want, rtol=0, atol=1e-12) and refined['scale'] == rdet['scale']
    for key in ('ate_rmse', 'rot_err_mean_deg', 'rot_err_max_deg'):
        assert refined[key] <= plain[key], key
    assert all(a >= b for a, b in zip(refined['fscore'], plain['fscore'])) and refined['overall'] <= plain['overall']
    centre = np.mean([x['pts3d'][x['valid_mask']].mean(axis=0) for x in views], axis=0).astype(np.float64)
    turn = similarity((1, 2, 3), 2.0, 1.0, (0, 0, 0))
    turn[:3, 3] = centre - turn[:3, :3] @ centre
    off = evaluate_scene(aligned, views, align=turn @ det['similarity'], thresholds=th)
    mended, mdet = evaluate_scene(aligned, views, align=turn @ det['similarity'], thresholds=th, refine='icp', return_details=True)
    _report(off, 'turned, refine=None'), _report(mended, "turned, refine='icp'")
    assert mdet['refined'] is True and mdet['registration'].converged and mended['voxel_size'] == v
    assert np.allclose(mdet['similarity'], mdet['registration'].similarity @ turn @ det['similarity'], rtol=0, atol=1e-12)
    for key in ('ate_rmse', 'rot_err_mean_deg', 'rot_err_max_deg'):
        assert mended[key] < off[key], key
    assert all(a > b for a, b in zip(mended['fscore'], off['fscore'])) and mended['overall'] < off['overall']
    with pytest.raises(ValueError, match="refine is 'icp' or None"):
        evaluate_scene(aligned, views, refine='ransac')


# ---- 5. the command line --------------------------------------------------------------------------------------------------------------------
def test_command_line_register(gpu, tmp_path, capsys):
    """two PLYs of the scene: --register recovers the similarity to the end-to-end bar (the restatement run with the PCA normals of
    k = 16 that the command computes for a cloud without normals); --init and --rigid are passed on; without --register the line is
    cloud_metrics of the raw files"""
    from dust3r_amd.cloud_metrics import cloud_metrics
    from dust3r_amd.evaluation import main
    from dust3r_amd.export import write_ply
    src, dst, _ = scene('fresh')
    grey = np.full((1, 3), 128, np.uint8)
    paths = [write_ply(str(tmp_path / name), pts, np.repeat(grey, len(pts), axis=0)) for name, pts in (('pred.ply', src), ('gt.ply', dst))]
    stages = [str(s) for s in STAGES]
    assert main(paths + ['--max-dist', '0.03']) == 0
    assert json.loads(capsys.readouterr().out) == json.loads(json.dumps(cloud_metrics(src, dst, 0.03, [0.03 / 16, 0.03 / 8, 0.03 / 4])))
    assert main(paths + ['--max-dist', '0.03', '--register', '--register-dist'] + stages) == 0
    line = json.loads(capsys.readouterr().out)
    normals16 = pca_normals(dst, k=16)
    assert_end_to_end_bar(np.array(line['similarity']), line['registration_pairs'], restated_register(src, dst, normals16, STAGES), 'command line')
    raw = cloud_metrics(src, dst, 0.03, [0.03 / 16, 0.03 / 8, 0.03 / 4])
    assert line['registration_rmse'] > 0 and line['n_found_pred'] >= line['registration_pairs'] and line['overall'] < raw['overall']
    assert set(line) == set(raw) | {'similarity', 'registration_rmse', 'registration_pairs'}
    np.savetxt(str(tmp_path / 'init.txt'), RIGID_INIT)
    assert main(paths + ['--max-dist', '0.03', '--register', '--rigid', '--init', str(tmp_path / 'init.txt'), '--register-dist'] + stages) == 0
    rigid = json.loads(capsys.readouterr().out.splitlines()[-1])                      # behind what the bar above printed
    assert_end_to_end_bar(np.array(rigid['similarity']), rigid['registration_pairs'],
                          restated_register(src, dst, normals16, STAGES, init=RIGID_INIT, with_scale=False), 'command line, rigid', rigid=True)


# ---- 6. the resource report -----------------------------------------------------------------------------------------------------------------
def test_resource_report_has_no_scratch():
    """read only: the report is what the build left next to the object; nothing is built or touched here"""
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'cloud_icp.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no cloud_icp.resources.txt: the library was not built by dust3r_amd/build.py')
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    new = [k for k in kernels if 'cloud_icp' in k or 'cloud_transform' in k or 'cloud_sums_final' in k]
    assert len(new) == 5 and sum('cloud_icp_sums_kernel' in k for k in new) == 2 and sum('cloud_sums_final_kernel' in k for k in new) == 2
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
