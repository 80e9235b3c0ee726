"""Global cloud registration on the GPU (csrc/cloud_features.hip, cloud_metrics.global_registration) against the numpy restatements of
tests/test_cloud_global_cpu.py. Every kernel is run on the restatement's inputs for its stage, so a difference in one stage cannot hide
in the next: the grid heads, SPFH, FPFH, the feature search and the RANSAC; then the composition end to end against the truth."""
import json
import os
import re

import numpy as np
import pytest
import torch

from test_cloud_global_cpu import (DIM, GLOBAL_BAR, KINDS, REFINED_BARS, TRUTH, bumpy, restated_case, restated_feature_nearest, restated_fpfh,
                                   restated_grid_heads, brute_force_knn, restated_ransac, restated_spfh, scene)
from test_cloud_icp_cpu import STAGES, pca_normals, similarity, similarity_distance

pytestmark = pytest.mark.gpu

F32 = np.float32


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(a):
    a = np.ascontiguousarray(a, F32)
    return np.where(np.isnan(a), np.uint32(0x7FC00000), a.view(np.uint32))


# ---- 1. the grid heads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 64, 65, 70001])
def test_grid_heads_are_the_lowest_index_of_every_cell(gpu, n):
    from dust3r_amd.cloud_metrics import grid_subsample
    rng = np.random.default_rng(n)
    P = (rng.standard_normal((n, 3)) * 3).astype(F32)
    if n > 1:
        P[n // 2:n // 2 + n // 8] = P[:n // 8]                                     # duplicates: the lower index is the head
        P[3::7, 0], P[5::11, 2] = np.nan, np.inf
    for cell in (0.25, 2.0):
        want = restated_grid_heads(P, cell)
        got = grid_subsample(_dev(P, gpu), cell)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n, cell)
        assert len(want) >= 1 and (n < 64 or len(want) < np.isfinite(P).all(axis=1).sum())      # some cell holds more than one point
    assert len(grid_subsample(_dev(np.full((5, 3), np.nan, F32), gpu), 1.0)) == 0


# ---- 2. SPFH and FPFH ------------------------------------------------------------------------------------------------------------------------
_STAGE = {}


def descriptor_inputs(n, k):
    """(P, N, d2, idx, counts, flagged) of the restatement on n points of the bumpy surface with outward PCA-free normals (the radial
    direction through the ellipsoid's metric), and the rows the issue names: -1 padding, a duplicate point (dist 0), a NaN normal, a zero
    normal, a neighbour exactly along the normal"""
    if (n, k) not in _STAGE:
        pts, u = bumpy(np.random.default_rng(100 + n), n)
        P = pts.astype(F32)
        N = (u / np.array([1.0, 0.8, 0.6]))
        N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(F32)
        if n > 16:
            P[5] = P[2]
            N[7, 1] = np.nan
            N[9] = 0
            N[11] = (0, 0, 1)
            P[12] = P[11] + np.array([0, 0, 0.25], F32)
        d2, idx = brute_force_knn(P, P, k, 0.5 if n > 100 else 4.0, exclude_self=True)
        if n > 16:
            idx[11, 0], d2[11, 0] = 12, F32(0.0625)
            idx[13, -1], d2[13, -1] = -1, np.inf
        counts, flagged = restated_spfh(P, N, idx)
        _STAGE[n, k] = (P, N, d2, idx, counts, flagged)
    return _STAGE[n, k]


@pytest.mark.parametrize('k', [1, 7, 32])
@pytest.mark.parametrize('n', [1, 63, 65, 1500])
def test_spfh_is_byte_equal_away_from_the_bin_edges(gpu, n, k):
    from dust3r_amd.cloud_metrics import spfh_counts
    P, N, _, idx, want, flagged = descriptor_inputs(n, k)
    got = spfh_counts(_dev(P, gpu), _dev(N, gpu), _dev(idx.astype(np.int32), gpu)).cpu().numpy()
    print(f'n = {n}, k = {k}: {flagged.mean():.2%} of the rows flagged, {np.abs(got.astype(int) - want).any(axis=1).sum()} rows differ')
    assert flagged.mean() <= 0.05                                                  # the exclusion cannot hide a broken kernel
    assert got.shape == (n, 36) and got.dtype == np.uint8
    assert np.array_equal(got[~flagged], want[~flagged])
    assert (got[:, DIM] == got[:, :11].sum(axis=1)).all() and (got[:, 34:] == 0).all()      # every pair lands in one bin of each feature
    assert (got[:, DIM] == got[:, 11:22].sum(axis=1)).all() and (got[:, DIM] == got[:, 22:33].sum(axis=1)).all()
    if n > 16:
        assert got[7, DIM] == 0 and got[9, DIM] == 0                              # a NaN normal, a zero normal: no pair
        assert got[11, DIM] == want[11, DIM] < (idx[11] >= 0).sum()               # the neighbour along the normal is skipped


@pytest.mark.parametrize('k', [1, 7, 32])
@pytest.mark.parametrize('n', [1, 63, 65, 1500])
def test_fpfh_is_bit_equal(gpu, n, k):
    from dust3r_amd.cloud_metrics import fpfh_features
    _, _, d2, idx, counts, _ = descriptor_inputs(n, k)
    counts = counts.copy()
    if n > 16:
        counts[idx[20][idx[20] >= 0]] = 0                                          # a row whose neighbours all have m = 0
    want = restated_fpfh(idx, d2, counts)
    got = fpfh_features(_dev(d2, gpu), _dev(idx.astype(np.int32), gpu), _dev(counts, gpu)).cpu().numpy()
    assert got.shape == (n, DIM) and np.array_equal(_bits(got), _bits(want))
    if n > 16 and counts[20, DIM] > 0:
        assert np.allclose(got[20].reshape(3, 11).sum(axis=1), 100, atol=1e-3)    # its own histogram alone
    live = want.reshape(n, 3, 11).sum(axis=2) > 0
    assert np.allclose(got.reshape(n, 3, 11).sum(axis=2)[live], 100, atol=1e-3)


# ---- 3. the feature search -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('na,nb', [(1, 1), (63, 257), (64, 64), (65, 1), (257, 63), (1500, 1500)])
def test_feature_nearest_is_bit_equal(gpu, na, nb):
    from dust3r_amd._lib import check, current_stream, lib, ptr
    rng = np.random.default_rng(1000 * na + nb)
    A, B = rng.uniform(0, 100, (na, DIM)).astype(F32), rng.uniform(0, 100, (nb, DIM)).astype(F32)
    if nb > 8:
        B[5] = B[2]                                                               # duplicate rows: the lowest index wins
        A[0] = B[2]
        B[3, 32], B[7, 0] = np.nan, np.inf
    if na > 8:
        A[4, 17], A[6, 32] = np.nan, -np.inf
        A[1] = B[nb - 1]                                                          # the last row of b is looked at
    PAD, SENT_D, SENT_I = 64, F32(-7.0), -12345
    for b_host in (B, np.full_like(B, np.nan)):
        want_d2, want_idx = restated_feature_nearest(A, b_host)
        d2 = torch.full((na + PAD,), float(SENT_D), dtype=torch.float32, device=gpu)
        idx = torch.full((na + PAD,), SENT_I, dtype=torch.int32, device=gpu)
        a, b = _dev(A, gpu), _dev(b_host, gpu)
        with torch.cuda.device(gpu):
            check(lib.d3r_feature_nearest(na, ptr(a), nb, ptr(b), ptr(d2), ptr(idx), current_stream()), 'feature_nearest')
        d2, idx = d2.cpu().numpy(), idx.cpu().numpy()
        assert np.array_equal(idx[:na], want_idx) and np.array_equal(_bits(d2[:na]), _bits(want_d2))
        assert (d2[na:] == SENT_D).all() and (idx[na:] == SENT_I).all()           # nothing is written behind the outputs
    assert (want_idx == -1).all() and np.isinf(want_d2).all()                     # b entirely NaN
    if nb > 8:
        want_d2, want_idx = restated_feature_nearest(A, B)
        assert want_idx[0] == 2 and want_d2[0] == 0 and want_idx[1] == nb - 1 and not np.isin(want_idx, [3, 7]).any()
    if na > 8:
        assert want_idx[4] == -1 and want_idx[6] == -1


def test_match_features_keeps_the_mutual_pairs(gpu):
    from dust3r_amd.cloud_metrics import match_features
    from test_cloud_global_cpu import restated_match
    rng = np.random.default_rng(5)
    A, B = rng.uniform(0, 100, (300, DIM)).astype(F32), rng.uniform(0, 100, (200, DIM)).astype(F32)
    A[:50] = B[:50] + rng.normal(0, 0.5, (50, DIM)).astype(F32)
    ia, ib = match_features(_dev(A, gpu), _dev(B, gpu))
    want = restated_match(A, B)
    assert np.array_equal(ia.cpu().numpy(), want[0]) and np.array_equal(ib.cpu().numpy(), want[1]) and len(want[0]) >= 50


# ---- 4. the RANSAC ---------------------------------------------------------------------------------------------------------------------------
def planted(n, scale, seed):
    """n correspondences of a planted similarity, the last third of them wrong"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, 3)).astype(F32)
    T = similarity((1, -1, 2), 75.0, scale, (0.5, 2.0, -1.0))
    q = (p.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F32)
    bad = n - n // 3 if n > 4 else n
    q[bad:] = rng.uniform(-4, 4, (n - bad, 3)).astype(F32)
    return p, q


def run_ransac(gpu, p, q, seed, n_hyp, thr, with_scale):
    from dust3r_amd.cloud_metrics import sim3_ransac
    best, inliers = sim3_ransac(_dev(p, gpu), _dev(q, gpu), n_hyp, thr, 0.9, with_scale, seed)
    return best.cpu().numpy(), inliers.cpu().numpy()


@pytest.mark.parametrize('with_scale', [True, False])
@pytest.mark.parametrize('n_corr', [3, 4, 64, 65, 510])
def test_ransac_equals_the_restatement(gpu, n_corr, with_scale):
    p, q = planted(n_corr, 1.7 if with_scale else 1.0, n_corr)
    if n_corr > 8:
        p[5, 1], q[6, 0] = np.nan, np.inf                                         # a non-finite correspondence is never an inlier
    thr, seed = 0.01, 9
    for n_hyp in (1, 255, 256, 257, 4096):
        want = restated_ransac(p, q, seed, n_hyp, thr, 0.9, with_scale)
        best, inliers = run_ransac(gpu, p, q, seed, n_hyp, thr, with_scale)
        print(f"n_corr {n_corr}, n_hyp {n_hyp}: h {want['h']}, count {want['count']}, valid {want['n_valid']}, margin {want['margin']:.3g}")
        assert want['margin'] > 1e-4                                               # no correspondence of the winner within rounding of the gate
        assert (int(best[0]), int(best[1]), int(best[2])) == (want['h'], want['count'], want['n_valid']), n_hyp
        assert np.array_equal(inliers.astype(bool), want['inliers'])
        assert np.abs(best[3:] - want['S']).max() <= 1e-12 * max(1.0, np.abs(want['S']).max())
    assert want['h'] >= 0 and want['count'] == (n_corr - n_corr // 3 - (2 if n_corr > 8 else 0) if n_corr > 4 else n_corr)


def test_ransac_without_a_valid_hypothesis_and_reproducibility(gpu):
    one = np.tile(np.array([[0.5, -1.0, 2.0]], F32), (40, 1))
    best, inliers = run_ransac(gpu, one, one, 0, 512, 0.1, True)
    assert best[0] == -1 and best[1] == 0 and best[2] == 0 and not best[3:].any() and not inliers.any()
    p, q = planted(200, 1.3, 1)
    a, b = run_ransac(gpu, p, q, 4, 4096, 0.01, True), run_ransac(gpu, p, q, 4, 4096, 0.01, True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[0][0] >= 0
    other = run_ransac(gpu, p, q, 5, 4096, 0.01, True)
    assert other[0][1] == a[0][1] == 134                                            # another seed: the same support


def test_ransac_on_the_matches_of_the_scene(gpu):
    """the correspondences the restated pipeline hands to its RANSAC, at the pipeline's own sizes"""
    g = restated_case('full')
    best, inliers = run_ransac(gpu, g['p'], g['q'], 0, 65536, g['thr'], True)
    want = g['ransac']
    print(f"margin {want['margin']:.3g}")
    assert (int(best[0]), int(best[1]), int(best[2])) == (want['h'], want['count'], want['n_valid'])
    assert np.array_equal(inliers.astype(bool), want['inliers']) and np.abs(best[3:] - want['S']).max() <= 1e-12 * np.abs(want['S']).max()


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
def test_register_clouds_from_a_global_start(gpu, kind):
    from dust3r_amd.cloud_metrics import register_clouds
    src, dst = scene(kind)
    details = {}
    reg = register_clouds(_dev(src, gpu), _dev(dst, gpu), STAGES, init='global', details=details)
    g = details['global']
    ang0, ds0, _ = similarity_distance(g.similarity, TRUTH)
    ang, ds, _ = similarity_distance(reg.similarity, TRUTH)
    print(f'{kind}: features {g.n_features}, matches {g.n_matches}, valid {g.n_valid}, inliers {g.n_inliers}, mirrored {g.mirrored}; global '
          f'{ang0:.3g} deg / {ds0:.3g}, after ICP {ang:.3g} deg / {ds:.3g}, {reg.iterations} iterations')
    assert g.reason is None and not g.mirrored and g.n_inliers >= 3 and g.best_hypothesis >= 0
    assert reg.converged
    assert ang <= REFINED_BARS[kind][0] and ds <= REFINED_BARS[kind][1]


def outward_normals(P):
    N = pca_normals(P, k=16)
    ok = np.isfinite(P).all(axis=1)
    c = P[ok].astype(np.float64).mean(axis=0)
    return np.where((((P - c) * N).sum(axis=1) >= 0)[:, None], N, -N).astype(F32)


def test_mirrored_run_recovers_negated_normals(gpu):
    from dust3r_amd.cloud_metrics import global_registration
    src, dst = scene('full')
    Ns, Nd = outward_normals(src), outward_normals(dst)
    plain = global_registration(_dev(src, gpu), _dev(dst, gpu), src_normals=Ns, dst_normals=Nd)
    flipped = global_registration(_dev(src, gpu), _dev(dst, gpu), src_normals=-Ns, dst_normals=Nd)
    alone = global_registration(_dev(src, gpu), _dev(dst, gpu), src_normals=-Ns, dst_normals=Nd, try_mirrored=False)
    print(f'plain {plain.n_inliers} inliers, flipped {flipped.n_inliers} (mirrored {flipped.mirrored}), without the mirrored run {alone.n_inliers}')
    assert not plain.mirrored and flipped.mirrored and not alone.mirrored
    ang, ds, _ = similarity_distance(flipped.similarity, TRUTH)
    assert ang <= GLOBAL_BAR[0] and ds <= GLOBAL_BAR[1]
    assert alone.n_inliers < flipped.n_inliers


def test_fused_cloud_feature_cloud(gpu):
    from dust3r_amd.viz import FusedCloud
    from test_cloud_global_cpu import restated_feature_cloud
    dst = scene('full')[1]
    N = outward_normals(dst)
    cloud = FusedCloud(dst, None, None, None, voxel_size=float('nan'), bounds=(dst.min(axis=0), dst.max(axis=0)), normals=N)
    P, Nf = cloud.feature_cloud(cell=0.12)
    want = restated_feature_cloud(dst, N, cell=0.12)
    assert isinstance(P, np.ndarray) and np.array_equal(P, want[0]) and np.array_equal(Nf, want[1])      # the cloud's own normals, at the heads
    assert len(cloud.feature_cloud()[0]) == len(restated_feature_cloud(dst, N)[0])                        # the default cell: 0.1 of the size
    bare = FusedCloud(_dev(dst, gpu), None, None, None, voxel_size=float('nan'), bounds=cloud.bounds)
    P, Nf = bare.feature_cloud(cell=0.12)
    assert isinstance(P, torch.Tensor) and np.array_equal(P.cpu().numpy(), want[0])
    P, Nf = P.double(), Nf.double()
    assert (((P - P.mean(dim=0)) * Nf).sum(dim=1) >= 0).all() and torch.allclose(Nf.norm(dim=1), torch.ones(len(Nf), dtype=torch.float64, device=gpu), atol=1e-5)


def test_too_few_matches_give_a_reason(gpu):
    from dust3r_amd.cloud_metrics import global_registration
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], F32)
    res = global_registration(_dev(P, gpu), _dev(P * 2, gpu), n_hyp=64)
    assert res.similarity is None and res.reason and res.best_hypothesis == -1


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------------------
def test_command_line_global(gpu, tmp_path, capsys):
    from dust3r_amd.cloud_metrics import cloud_metrics
    from dust3r_amd.evaluation import main
    from dust3r_amd.export import write_ply
    src, dst = scene('full')
    grey = np.full((1, 3), 128, np.uint8)
    paths = [write_ply(str(tmp_path / name), pts, np.repeat(grey, len(pts), axis=0)) for name, pts in (('pred.ply', src), ('gt.ply', dst))]
    stages = [str(s) for s in STAGES]
    assert main(paths + ['--max-dist', '0.03']) == 0
    raw = json.loads(capsys.readouterr().out)
    assert raw == json.loads(json.dumps(cloud_metrics(src, dst, 0.03, [0.03 / 16, 0.03 / 8, 0.03 / 4])))      # without --global: the line it was
    assert main(paths + ['--max-dist', '0.03', '--register', '--global', '--seed', '0', '--ransac-iters', '65536', '--register-dist'] + stages) == 0
    line = json.loads(capsys.readouterr().out)
    assert set(line) == set(raw) | {'similarity', 'registration_rmse', 'registration_pairs', 'global_similarity', 'global_inliers', 'global_matches'}
    ang, ds, _ = similarity_distance(np.array(line['similarity']), TRUTH)
    ang0, ds0, _ = similarity_distance(np.array(line['global_similarity']), TRUTH)
    print(f'global {ang0:.3g} deg / {ds0:.3g}, registered {ang:.3g} deg / {ds:.3g}')
    assert ang <= REFINED_BARS['full'][0] and ds <= REFINED_BARS['full'][1]
    assert line['global_inliers'] >= 3 and line['global_matches'] >= line['global_inliers']
    assert raw['n_found_pred'] < 100 and line['n_found_pred'] > 2000              # the raw files share no frame; the registered ones do
    np.savetxt(str(tmp_path / 'init.txt'), TRUTH)
    assert main(paths + ['--max-dist', '0.03', '--register', '--init', str(tmp_path / 'init.txt'), '--register-dist'] + stages) == 0
    assert set(json.loads(capsys.readouterr().out.splitlines()[-1])) == set(raw) | {'similarity', 'registration_rmse', 'registration_pairs'}      # behind the print above


# ---- 7. the resource report ------------------------------------------------------------------------------------------------------------------
def test_resource_report_has_no_scratch():
    """read only: the report is what the build left next to the object"""
    from dust3r_amd import _lib
    report = open(os.path.join(os.path.dirname(_lib.LIB_PATH), 'cloud_features.resources.txt')).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    own = [k for k in kernels if any(s in k for s in ('grid_heads', 'spfh', 'fpfh', 'feature_nearest', 'sim3_'))]
    assert len(own) == 8
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
