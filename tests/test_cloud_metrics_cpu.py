"""Cloud-to-cloud metrics without a GPU: the numpy restatements that tests/test_cloud_metrics_gpu.py holds the kernels of csrc/cloud_nn.hip
against, checked here against each other and against SciPy.
- `brute_force`: THE definition (include/dust3r_hip.h): chunked fp32 numpy over all pairs, d2 = (dx dx + dy dy) + dz dz with every operation
  rounded on its own (numpy never contracts), the lowest index of the minimum, accepted when <= r r (fp32).
- `restated_grid_nearest`: the same minimum, but looking only at the reference points whose cell lies in the padded cell range of the
  query -- the argument of DESIGN.md ("Cloud metrics") that the grid cannot lose a point within r, restated and tried on the inputs that
  would break it: lattices with many distances exactly r, ties, offsets where one ulp exceeds r, cells of r / 2, r and 2 r."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = np.float32(1 + 2.0 ** -10)


def valid_rows(P):
    return np.isfinite(P).all(axis=1)


def brute_force(Q, R, r, chunk=256):
    """(d2 float32, idx int32) of the definition; Q (n, 3), R (m, 3) float32"""
    Q, R, r = np.asarray(Q, np.float32).reshape(-1, 3), np.asarray(R, np.float32).reshape(-1, 3), np.float32(r)
    r2 = r * r
    rows = np.flatnonzero(valid_rows(R))
    Rv = R[rows]
    d2_out, idx_out = np.full(len(Q), np.inf, np.float32), np.full(len(Q), -1, np.int32)
    if len(Rv) == 0:
        return d2_out, idx_out
    for s in range(0, len(Q), chunk):
        q = Q[s:s + chunk]
        ok = valid_rows(q)
        with np.errstate(over='ignore', invalid='ignore'):
            d = np.where(ok[:, None], q, np.float32(0))[:, None, :] - Rv[None, :, :]
            m = d * d
            d2 = (m[..., 0] + m[..., 1]) + m[..., 2]
        assert d2.dtype == np.float32
        j = d2.argmin(axis=1)                                          # the first of the minima: the lowest index
        best = d2[np.arange(len(q)), j]
        found = ok & (best <= r2)
        d2_out[s:s + chunk][found] = best[found]
        idx_out[s:s + chunk][found] = rows[j[found]]
    return d2_out, idx_out


def axis_f(x, lo, cell):
    with np.errstate(over='ignore', invalid='ignore'):
        return np.floor((np.asarray(x, np.float32) - np.float32(lo)) / np.float32(cell))


def restated_grid_nearest(Q, R, r, cell):
    """The grid search in numpy: cells by key_of's arithmetic from the minimum of the valid reference points, per query the padded range
    q(nextafter(a - r', -inf)) .. q(nextafter(a + r', +inf)), r' = r (1 + 2^-10); only reference points in those cells are looked at.
    Returns (d2, idx, evaluations per query)."""
    from dust3r_amd.viz import fuse_key_bits
    Q, R, r, cell = np.asarray(Q, np.float32), np.asarray(R, np.float32), np.float32(r), np.float32(cell)
    r2, rp = r * r, r * PAD
    rows = np.flatnonzero(valid_rows(R))
    Rv = R[rows]
    d2_out, idx_out, evals = np.full(len(Q), np.inf, np.float32), np.full(len(Q), -1, np.int32), np.zeros(len(Q), np.int64)
    if len(Rv) == 0:
        return d2_out, idx_out, evals
    lo, hi = Rv.min(axis=0), Rv.max(axis=0)
    qmax = np.float32([2 ** b - 1 for b in fuse_key_bits(lo, hi, cell)])
    cells = np.stack([np.clip(axis_f(Rv[:, c], lo[c], cell), 0, qmax[c]) for c in range(3)], axis=1)
    inf = np.float32(np.inf)
    for i in np.flatnonzero(valid_rows(Q)):
        a = Q[i]
        with np.errstate(over='ignore'):
            f0 = np.array([axis_f(np.nextafter(a[c] - rp, -inf), lo[c], cell) for c in range(3)], np.float32)
            f1 = np.array([axis_f(np.nextafter(a[c] + rp, inf), lo[c], cell) for c in range(3)], np.float32)
        if (f1 < 0).any() or (f0 > qmax).any():
            continue
        c0, c1 = np.clip(f0, 0, qmax), np.clip(f1, 0, qmax)
        look = ((cells >= c0) & (cells <= c1)).all(axis=1)
        evals[i] = look.sum()
        if not look.any():
            continue
        with np.errstate(over='ignore'):
            d = a[None, :] - Rv[look]
            m = d * d
            d2 = (m[:, 0] + m[:, 1]) + m[:, 2]
        j = d2.argmin()
        if d2[j] <= r2:
            d2_out[i], idx_out[i] = d2[j], rows[np.flatnonzero(look)[j]]
    return d2_out, idx_out, evals


def lattice_case(rng, r, offset, side=5):
    """A reference lattice of spacing r at `offset` (fp32: at a large offset the lattice collapses onto the few representable numbers, where
    one ulp exceeds r) with duplicates, and queries ON lattice sites (distance 0 and ties), exactly r and 2 r beside them, one and two
    spacings outside every face, and a few random ones."""
    r = np.float32(r)
    g = np.arange(side, dtype=np.float32)
    site = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    R = (np.float32(offset) + site * r).astype(np.float32)
    R = np.concatenate([R, R[rng.integers(0, len(R), 20)]])                              # duplicates: the lowest index wins
    R = R[rng.permutation(len(R))]
    Q = [R[rng.integers(0, len(R), 30)]]
    for axis in range(3):
        for k in (-2, -1, 1, 2):
            e = np.zeros(3, np.float32)
            e[axis] = k
            Q.append((np.float32(offset) + (site[rng.integers(0, len(site), 12)] + e) * r).astype(np.float32))
            face = site[site[:, axis] == (0 if k < 0 else side - 1)][:6]
            Q.append((np.float32(offset) + (face + e) * r).astype(np.float32))           # outside the face
    Q.append((np.float32(offset) + rng.random((30, 3)).astype(np.float32) * (side + 2) * r - r).astype(np.float32))
    half = np.float32(offset) + (site[:20] + np.float32(0.5)) * r                         # cell centres: eight-fold ties
    Q.append(half.astype(np.float32))
    return np.concatenate(Q).astype(np.float32), R


OFFSETS = (0.0, 1000.0, -37.3, 5e4)
CELLS = (0.5, 1.0, 2.0)


@pytest.mark.parametrize('offset', OFFSETS)
def test_grid_restatement_equals_brute_force_on_lattices(offset):
    rng = np.random.default_rng(int(abs(offset)) + 1)
    for r in (1e-3, 0.25):
        Q, R = lattice_case(rng, r, offset)
        want = brute_force(Q, R, r)
        if offset == 0.0:
            assert (want[0] == np.float32(r) * np.float32(r)).any() and (want[0] == 0).any() and (want[1] < 0).any()
        for factor in CELLS:
            got = restated_grid_nearest(Q, R, r, np.float32(r) * np.float32(factor))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (offset, r, factor)


def test_grid_restatement_on_random_clouds_and_nonfinite_points():
    rng = np.random.default_rng(5)
    R = (rng.random((1500, 3)) * np.float32([4, 2, 0])).astype(np.float32)               # planar: one axis has a single cell
    Q = (rng.random((700, 3)) * np.float32([5, 3, 0.3]) - np.float32([0.5, 0.5, 0.15])).astype(np.float32)
    R[::97, 1] = np.nan
    Q[::89, 0] = np.inf
    want = brute_force(Q, R, 0.1)
    assert (want[1] >= 0).sum() > 100 and (want[1] < 0).sum() > 100
    for cell in (0.05, 0.1, 0.2, 50.0):
        got = restated_grid_nearest(Q, R, 0.1, cell)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), cell
    assert (restated_grid_nearest(Q, R, 0.1, 0.1)[2].mean() < 0.1 * len(R))             # and it looks at a fraction of the cloud


def test_brute_force_against_ckdtree():
    """The restatement against SciPy's KD-tree in fp64 on the same fp32 points. First, on the fp64 reference alone: no nearest distance lies
    within a relative 1e-5 of max_dist, so the found sets cannot differ by rounding; then they are identical, every query included.
    d2 carries three fp32 product roundings, three subtraction roundings (doubled by the square) and two sums: below 2^-21 relative."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(11)
    R, Q = rng.random((3000, 3)).astype(np.float32), rng.random((2500, 3)).astype(np.float32)
    max_dist = 0.05
    dist, nn = cKDTree(R.astype(np.float64)).query(Q.astype(np.float64))
    assert not (np.abs(dist - max_dist) <= 1e-5 * max_dist).any()
    found = dist <= max_dist
    assert 500 < found.sum() < len(Q) - 500
    d2, idx = brute_force(Q, R, max_dist)
    assert np.array_equal(idx >= 0, found)
    assert np.array_equal(idx[found], nn[found])                                          # (no ties in a random cloud)
    assert np.all(np.abs(d2[found].astype(np.float64) - dist[found] ** 2) <= 2.0 ** -21 * dist[found] ** 2)
    assert np.all(np.isinf(d2[~found]))


def test_ladder_radii_and_cells():
    from dust3r_amd.cloud_metrics import grid_cell, ladder_radii
    rs = ladder_radii(0.01, 1.0)
    assert [float(x) for x in rs] == [float(np.float32(v)) for v in (0.01, 0.04, 0.16, 0.64)] + [1.0] and all(x.dtype == np.float32 for x in rs)
    assert ladder_radii(2.0, 2.0) == [np.float32(2.0)] and ladder_radii(0.5, 2.0)[-1] == np.float32(2.0)
    for bad in (0.0, -1.0, float('nan'), float('inf'), 1e-20, 1e20):      # the last two: r r is subnormal / infinite in float32
        with pytest.raises(ValueError):
            ladder_radii(bad, 1.0)
        with pytest.raises(ValueError):
            ladder_radii(1.0, bad)
    cell, bits = grid_cell(np.float32([0, 0, 0]), np.float32([1e5, 1, 0]), 1e-3)          # 1e8 cells of r along x: doubled until 21 bits hold
    assert bits[0] == 21 and bits[2] == 1 and cell == np.float32(1e-3) * 2 ** 6


def test_metric_composition_from_hand_made_counts():
    from dust3r_amd.cloud_metrics import compose_metrics
    pred = dict(n_valid=10, n_found=8, sum_d=4.0, sum_d2=3.0, median_d2=0.25, counts=[2, 8])
    gt = dict(n_valid=20, n_found=5, sum_d=1.0, sum_d2=0.5, median_d2=0.04, counts=[0, 5])
    m = compose_metrics(pred, gt, [0.1, 1.0])
    assert m['accuracy'] == 0.5 and m['completeness'] == 0.2 and m['overall'] == 0.35
    assert m['accuracy_median'] == 0.5 and m['completeness_median'] == 0.2
    assert m['precision'] == [0.2, 0.8] and m['recall'] == [0.0, 0.25]
    assert m['fscore'][0] == 0.0 and m['fscore'][1] == 2 * 0.8 * 0.25 / (0.8 + 0.25)
    assert math.isclose(m['outliers_pred'], 0.2) and m['outliers_gt'] == 0.75
    assert m['n_valid_pred'] == 10 and m['n_found_gt'] == 5 and m['counts_pred'] == [2, 8] and m['sum_d2_gt'] == 0.5 and m['thresholds'] == [0.1, 1.0]
    # nothing found on one side: its mean and median are NaN, and so is the Chamfer mean; precision and recall are 0, the F-score 0 (P + R = 0)
    none = dict(n_valid=10, n_found=0, sum_d=0.0, sum_d2=0.0, median_d2=float('nan'), counts=[0, 0])
    m = compose_metrics(none, none, [0.1, 1.0])
    assert all(math.isnan(m[k]) for k in ('accuracy', 'accuracy_median', 'completeness', 'completeness_median', 'overall'))
    assert m['precision'] == [0.0, 0.0] and m['fscore'] == [0.0, 0.0] and m['outliers_pred'] == 1.0
    m = compose_metrics(pred, none, [0.1, 1.0])
    assert m['accuracy'] == 0.5 and math.isnan(m['completeness']) and math.isnan(m['overall']) and m['fscore'] == [0.0, 0.0]
    # an empty cloud: no valid point, the ratios are NaN
    empty = dict(n_valid=0, n_found=0, sum_d=0.0, sum_d2=0.0, median_d2=float('nan'), counts=[0])
    m = compose_metrics(empty, empty, [0.1])
    assert math.isnan(m['precision'][0]) and math.isnan(m['outliers_gt'])


def test_exports_are_registered_and_refuse_bad_sizes():
    from dust3r_amd import _lib
    lib = _lib.lib
    assert lib.d3r_cloud_grid_workspace_bytes(0, 10) == 0 and lib.d3r_cloud_grid_workspace_bytes(10, 0) == 0 and lib.d3r_cloud_grid_workspace_bytes(-1, -1) == 0
    # two key and two index buffers per side (24 bytes a point) and the grid's float4, key and start (28 bytes a reference point)
    assert 52 * 10 ** 6 <= lib.d3r_cloud_grid_workspace_bytes(10 ** 6, 1) < 53 * 10 ** 6
    assert 25 * 10 ** 6 <= lib.d3r_cloud_grid_workspace_bytes(1, 10 ** 6) < 26 * 10 ** 6
    assert lib.d3r_cloud_distance_stats_workspace_bytes(0) == 0 and 0 < lib.d3r_cloud_distance_stats_workspace_bytes(10 ** 7) < 2 ** 20
    for name in ('d3r_cloud_grid_build', 'd3r_cloud_nearest', 'd3r_cloud_distance_stats'):
        assert hasattr(lib, name)


def _two_plys(tmp_path):
    from dust3r_amd.export import write_ply
    rng = np.random.default_rng(2)
    a = rng.random((200, 3)).astype(np.float32)
    b = (a + 0.01 * rng.standard_normal((200, 3))).astype(np.float32)
    colors = np.zeros((200, 3), np.uint8)
    return write_ply(str(tmp_path / 'pred.ply'), a, colors), write_ply(str(tmp_path / 'gt.ply'), b, colors), a, b


def test_command_line(tmp_path):
    """parsing, and what the command does where there is no device: the error every GPU entry point raises. With a device it prints the dict."""
    import torch
    from dust3r_amd import evaluation
    pred, gt, a, b = _two_plys(tmp_path)
    for argv in ([pred], [pred, gt], [pred, gt, '--max-dist', 'far'], [pred, gt, '--max-dist', '0.1', '--thresholds', 'x']):
        with pytest.raises(SystemExit) as e:
            evaluation.main(argv)
        assert e.value.code == 2, argv
    with pytest.raises(FileNotFoundError):
        evaluation.main([str(tmp_path / 'missing.ply'), gt, '--max-dist', '0.1'])
    r = subprocess.run([sys.executable, '-m', 'dust3r_amd.evaluation', pred, gt, '--max-dist', '0.1', '--thresholds', '0.01', '0.05'], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    if not torch.cuda.is_available():
        assert r.returncode != 0 and 'D3RError' in r.stderr and 'gfx950' in r.stderr
        return
    assert r.returncode == 0, r.stderr[-3000:]
    m = json.loads(r.stdout.strip().splitlines()[-1])
    d2, idx = brute_force(a, b, 0.1)
    assert m['n_valid_pred'] == 200 and m['n_found_pred'] == int((idx >= 0).sum()) and m['thresholds'] == [0.01, 0.05]
    assert m['counts_pred'] == [int((d2 <= np.float32(t) * np.float32(t)).sum()) for t in (0.01, 0.05)]


def test_evaluate_scene_refuses_a_cpu_scene():
    """a scene on the CPU: the error of every GPU entry point, before anything of the scene is read; a bad `align` is refused first"""
    import types
    import torch
    from dust3r_amd import _lib
    from dust3r_amd.evaluation import evaluate_scene, pose_errors
    scene = types.SimpleNamespace(device=torch.device('cpu'))
    with pytest.raises(_lib.D3RError, match='evaluate_scene runs on the GPU'):
        evaluate_scene(scene, [])
    with pytest.raises(ValueError, match="align is 'points', 'poses' or None"):
        evaluate_scene(scene, [], align='icp')
    # the pose errors by hand: a quarter turn about z and a shift of (3, 4, 0) on one of two cameras
    a = np.tile(np.eye(4), (2, 1, 1))
    b = a.copy()
    b[1, :3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    b[1, :3, 3] = [3, 4, 0]
    ate, mean, worst = pose_errors(a, b)
    assert math.isclose(ate, math.sqrt(25 / 2)) and math.isclose(mean, 45.0) and math.isclose(worst, 90.0)
    # near zero the angle keeps its digits (arccos of the trace would return 0 or 2e-8 here); at a half turn it is 180
    for angle in (1e-9, 3e-7, 1e-3):
        b = a.copy()
        b[0, :3, :3] = [[math.cos(angle), -math.sin(angle), 0], [math.sin(angle), math.cos(angle), 0], [0, 0, 1]]
        assert math.isclose(math.radians(pose_errors(a, b)[2]), angle, rel_tol=1e-6), angle
    b = a.copy()
    b[0, :3, :3] = np.diag([-1.0, -1.0, 1.0])
    assert math.isclose(pose_errors(a, b)[2], 180.0)


def test_entry_points_raise_without_a_device():
    import torch
    from dust3r_amd import _lib
    from dust3r_amd.cloud_metrics import cloud_metrics, nearest_in_cloud
    from dust3r_amd.viz import FusedCloud
    pts = np.zeros((4, 3), np.float32)
    if torch.cuda.is_available():                                      # with a device the same calls answer (four equal points: the lowest index)
        assert nearest_in_cloud(pts, pts, 1.0)[1].tolist() == [0, 0, 0, 0]
        return
    with pytest.raises(_lib.D3RError):
        nearest_in_cloud(pts, pts, 1.0)
    with pytest.raises(_lib.D3RError):
        cloud_metrics(pts, pts, 1.0, [0.5])
    cloud = FusedCloud(pts, np.zeros((4, 3), np.uint8), np.ones(4, np.float32), np.ones(4, np.int32), 0.1, (pts[0], pts[0]))
    with pytest.raises(_lib.D3RError):
        cloud.distance_to(cloud, 1.0)
