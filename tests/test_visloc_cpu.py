"""CPU tests (-m "not gpu") of the visual-localization package: dust3r_amd.visloc.evaluation against restatements written here with
SciPy's Rotation, the binding of the reference's visloc.py imports through the INTEGRATION.md aliases, the host build of the shared
P3P / stopping-rule math of csrc/visloc.hip, OpenCV's undistortion loop, the homogeneous geotrf, and the kernels' resource report."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation

from dust3r_amd import _lib
from dust3r_amd.utils.geometry import geotrf
from dust3r_amd.visloc import aggregate_stats, export_results, get_pose_error, undistort_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def _c2w(rng):
    T = np.eye(4)
    T[:3, :3] = Rotation.random(random_state=rng).as_matrix()
    T[:3, 3] = rng.normal(size=3) * 3
    return T


# ---- evaluation -----------------------------------------------------------------------------------------------------------------
def test_get_pose_error_matches_scipy_restatement():
    rng = np.random.RandomState(0)
    for k in range(200):
        a = _c2w(rng)
        b = a.copy() if k % 10 == 0 else _c2w(rng)
        if k % 3 == 1:                                     # small perturbations, where acos is least precise
            b[:3, :3] = Rotation.from_rotvec(rng.normal(size=3) * 1e-2).as_matrix() @ a[:3, :3]
        t_err, r_err = get_pose_error(a, b)
        assert isinstance(t_err, torch.Tensor) and t_err.dtype == torch.float64
        assert abs(float(t_err) - np.linalg.norm(a[:3, 3] - b[:3, 3])) < 1e-12
        ref = np.degrees(Rotation.from_matrix(a[:3, :3].T @ b[:3, :3]).magnitude())
        assert abs(float(r_err) - ref) < 2e-5, (k, float(r_err), ref)


def test_aggregate_stats_text():
    pose_errors = [0.05, 0.2, 0.3, 4.0, float('inf'), 0.09]
    angular_errors = [0.5, 1.5, 4.0, 9.0, float('inf'), 1.2]
    out = aggregate_stats('Cambridge', pose_errors, angular_errors)
    med_p, med_a = np.median(pose_errors), np.median(angular_errors)
    expected = f'Cambridge: 6 images - median_pos_error={med_p!r}, median_angular_error={med_a!r}'
    for (t, a), hits in zip([(0.1, 1), (0.25, 2), (0.5, 5), (5, 10)], [1, 3, 4, 5]):
        name = f'acc@{t:g}m,{a}deg'
        expected += '  - ' + name.ljust(12) + '=' + '%.3f' % (100 * hits / 6)
    assert out == expected
    assert out.endswith('  - acc@0.1m,1deg=16.667  - acc@0.25m,2deg=50.000  - acc@0.5m,5deg=66.667  - acc@5m,10deg=83.333')


def test_export_results_lines(tmp_path):
    rng = np.random.RandomState(1)
    names = ['seq1/frame00001.png', 'seq2/frame00042.png', 'frame7.png']
    poses = [_c2w(rng), None, _c2w(rng)]
    export_results(str(tmp_path), 'tol_conf_3.0_reproj_err_5.0', names, poses)
    assert export_results(None, 'x', names, poses) is None
    full = open(tmp_path / 'tol_conf_3.0_reproj_err_5.0_results.txt').read().splitlines()
    ltvl = open(tmp_path / 'tol_conf_3.0_reproj_err_5.0_ltvl.txt').read().splitlines()
    assert len(full) == len(ltvl) == 3
    for name, c2w, lf, ll in zip(names, poses, full, ltvl):
        f, lt = lf.split(' '), ll.split(' ')
        assert f[0] == name and lt[0] == os.path.basename(name) and f[1:] == lt[1:] and len(f) == 8
        w2c = np.eye(4) if c2w is None else np.linalg.inv(c2w)
        xyzw = Rotation.from_matrix(w2c[:3, :3]).as_quat()
        wxyz = np.array([xyzw[3], *xyzw[:3]])
        wxyz = -wxyz if wxyz[0] < 0 else wxyz
        vals = np.array([float(v) for v in f[1:]])
        assert np.abs(vals[:4] - wxyz).max() < 1e-12
        assert f[5:] == [str(v) for v in w2c[:3, 3].tolist()]


# ---- the reference's visloc.py through the aliases -------------------------------------------------------------------------------
def test_reference_visloc_binds_to_the_engine_through_the_integration_aliases():
    """with the dust3r.* hot-path modules and dust3r_visloc.localization / .evaluation aliased to this package,
    every name the reference's visloc.py imports from them (tests/golden/visloc_imports.json, tools/make_visloc_golden.py) is this
    package's object. The import statements run in a fresh interpreter."""
    imports = json.load(open(os.path.join(GOLD, 'visloc_imports.json')))['imports']
    assert {n for _, names in imports for n in names} >= {'inference', 'find_reciprocal_matches', 'geotrf', 'xy_grid', 'run_pnp',
                                                          'get_pose_error', 'aggregate_stats', 'export_results'}
    stmts = '\n'.join(f"from {mod} import {', '.join(names)}" for mod, names in imports)
    code = r"""
import sys, types
sys.path.insert(0, %r)
import dust3r_amd, dust3r_amd.model, dust3r_amd.inference, dust3r_amd.utils.geometry, dust3r_amd.visloc
import dust3r_amd.visloc.localization, dust3r_amd.visloc.evaluation
for pkg in ('dust3r', 'dust3r.utils', 'dust3r_visloc'):
    m = types.ModuleType(pkg)
    m.__path__ = []
    sys.modules[pkg] = m
for name in ('model', 'inference', 'utils.geometry'):
    sys.modules['dust3r.' + name] = sys.modules['dust3r_amd.' + name]
for name in ('localization', 'evaluation'):
    sys.modules['dust3r_visloc.' + name] = sys.modules['dust3r_amd.visloc.' + name]
%s
import dust3r_amd.visloc as V, dust3r_amd.utils.geometry as G, dust3r_amd.inference as I
assert run_pnp is V.localization.run_pnp and get_pose_error is V.evaluation.get_pose_error
assert aggregate_stats is V.evaluation.aggregate_stats and export_results is V.evaluation.export_results
assert find_reciprocal_matches is G.find_reciprocal_matches and geotrf is G.geotrf and xy_grid is G.xy_grid and inference is I.inference
print('aliases ok')
""" % (ROOT, stmts)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'aliases ok' in r.stdout, r.stderr[-2000:]


# ---- shared kernel math, host build ----------------------------------------------------------------------------------------------
def _dp(a):
    return a.ctypes.data_as(C.c_void_p)


def _project(w2c, X, fx, fy, cx, cy):
    Y = X @ w2c[:3, :3].T + w2c[:3, 3]
    return np.stack((fx * Y[:, 0] / Y[:, 2] + cx, fy * Y[:, 1] / Y[:, 2] + cy), axis=-1), Y[:, 2]


def test_p3p_recovers_the_pose_host():
    rng = np.random.RandomState(3)
    found = 0
    for k in range(300):
        w2c = np.linalg.inv(_c2w(rng))
        fx, fy, cx, cy = rng.uniform(300, 900), rng.uniform(300, 900), rng.uniform(200, 400), rng.uniform(150, 300)
        # points in front of the camera, in camera coordinates first
        Yc = np.c_[rng.uniform(-1, 1, (4, 2)) * 2, rng.uniform(2, 8, 4)]
        X = (Yc - w2c[:3, 3]) @ w2c[:3, :3]
        uv, z = _project(w2c, X, fx, fy, cx, cy)
        pose = np.zeros(12)
        ok = _lib.lib.d3r_selftest_p3p_host(_dp(np.ascontiguousarray(uv)), _dp(np.ascontiguousarray(X)), fx, fy, cx, cy, _dp(pose))
        assert ok == 1, k
        err = np.abs(pose.reshape(3, 4) - w2c[:3, :]).max() / max(1.0, np.abs(w2c[:3, 3]).max())
        found += err < 1e-6
    assert found >= 297, found          # a handful of near-degenerate draws may pick a different root at the fourth point's noise floor


def test_p3p_every_root_is_a_solution_host():
    rng = np.random.RandomState(4)
    for _ in range(200):
        X = rng.normal(size=(3, 3))
        w2c = np.linalg.inv(_c2w(rng))
        Y = X @ w2c[:3, :3].T + w2c[:3, 3]
        if (Y[:, 2] <= 0.5).any():
            continue
        f = Y / np.linalg.norm(Y, axis=1, keepdims=True)
        R, t = np.zeros((4, 9)), np.zeros((4, 3))
        n = _lib.lib.d3r_selftest_p3p_roots_host(_dp(np.ascontiguousarray(f)), _dp(np.ascontiguousarray(X)), _dp(R), _dp(t))
        assert 1 <= n <= 4
        truth = False
        for k in range(n):
            Rk = R[k].reshape(3, 3)
            assert np.abs(Rk @ Rk.T - np.eye(3)).max() < 1e-8 and abs(np.linalg.det(Rk) - 1) < 1e-8
            Yk = X @ Rk.T + t[k]
            fk = Yk / np.linalg.norm(Yk, axis=1, keepdims=True)
            assert np.abs(fk - f).max() < 1e-6                   # every root maps the three points onto their bearings
            truth |= np.abs(Rk - w2c[:3, :3]).max() < 1e-6 and np.abs(t[k] - w2c[:3, 3]).max() < 1e-6
        assert truth


def _update_num_iters(p, ep, model_points, max_iters):
    """OpenCV's RANSACUpdateNumIters, restated"""
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, sys.float_info.min)
    denom = 1.0 - (1.0 - ep) ** model_points
    if denom < sys.float_info.min:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if (denom >= 0 or -num >= max_iters * (-denom)) else int(np.rint(num / denom))


@pytest.mark.parametrize('ep', [0.0, 1e-9, 0.1, 0.3, 0.5, 0.6, 0.7, 0.9, 0.99, 1.0])
def test_ransac_stopping_rule_host(ep):
    for max_iters in (10_000, 355, 1):
        assert _lib.lib.d3r_selftest_ransac_iters_host(0.9999, ep, 4, max_iters) == _update_num_iters(0.9999, ep, 4, max_iters)


# ---- undistortion, geotrf ----------------------------------------------------------------------------------------------------------
def _opencv_undistort(uv, K, dist, iters=5):
    """cvUndistortPointsInternal (COUNT criteria, 4 coefficients, R = identity, P = K), one point at a time"""
    k1, k2, p1, p2 = dist
    out = []
    for u, v in uv:
        y0 = (v - K[1, 2]) / K[1, 1]
        x0 = (u - K[0, 2] - K[0, 1] * y0) / K[0, 0]
        x, y = x0, y0
        for _ in range(iters):
            r2 = x * x + y * y
            icdist = 1 / (1 + (k2 * r2 + k1) * r2)
            if icdist < 0:
                x, y = x0, y0
                break
            dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
            dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
            x, y = (x0 - dx) * icdist, (y0 - dy) * icdist
        h = K @ np.array([x, y, 1.0])
        out.append(h[:2] / h[2])
    return np.array(out)


def test_undistort_points_matches_opencv_loop():
    rng = np.random.RandomState(5)
    K = np.array([[600.0, 0, 330.5], [0, 580.0, 242.0], [0, 0, 1]])
    dist = [-0.12, 0.03, 0.001, -0.0007]
    uv = rng.uniform([0, 0], [640, 480], size=(500, 2))
    got = undistort_points(torch.from_numpy(uv), K, dist).numpy()
    assert np.abs(got - _opencv_undistort(uv, K, dist)).max() < 1e-9


def test_geotrf_homogeneous_matches_projective_formula_and_backends():
    rng = np.random.RandomState(6)
    H = np.array([[1.9, 0.01, 3.5], [-0.02, 2.1, -7.25], [1e-4, -2e-4, 1.0]])
    pts = rng.uniform(0, 512, size=(1000, 2))
    ref = np.c_[pts, np.ones(len(pts))] @ H.T
    ref = ref[:, :2] / ref[:, 2:]
    out = geotrf(H, pts, norm=True)
    assert out.shape == (1000, 2) and np.abs(out - ref).max() < 1e-9
    out_t = geotrf(torch.from_numpy(H), torch.from_numpy(pts), norm=True)
    assert np.array_equal(out_t.numpy(), out)                     # same bits from numpy and torch
    A = np.array([[2.0, 0, 0.5], [0, 2.0, -0.25], [0, 0, 1]])      # visloc's to_orig: affine
    assert np.abs(geotrf(A, pts, norm=True) - (2 * pts + [0.5, -0.25])).max() < 1e-12


def test_geotrf_homogeneous_batch():
    """a batch of (d+1)x(d+1) matrices with norm: the projective product per leading index, as the reference's non-einsum path"""
    rng = np.random.RandomState(7)
    H = rng.normal(size=(5, 3, 3))
    H[:, 2, 2] = 3.0
    for shape in ((5, 40, 2), (5, 2)):
        pts = rng.normal(size=shape)
        hom = np.concatenate([pts, np.ones(shape[:-1] + (1,))], -1)
        ref = np.einsum('bij,b...j->b...i', H, hom)
        ref = ref[..., :2] / ref[..., 2:]
        out = geotrf(H, pts, norm=True)
        assert out.shape == shape and np.abs(out - ref).max() < 1e-12
        assert np.array_equal(geotrf(torch.from_numpy(H), torch.from_numpy(pts), norm=True).numpy(), out)
    pts4 = torch.from_numpy(rng.normal(size=(5, 4, 6, 2)))      # torch (B, H, W, d): the reference's einsum path, affine + last coordinate
    aff = torch.einsum('bij,bhwj->bhwi', torch.from_numpy(H[:, :2, :2]), pts4) + torch.from_numpy(H[:, None, None, :2, 2])
    assert torch.allclose(geotrf(torch.from_numpy(H), pts4, norm=True), aff / aff[..., -1:], atol=1e-12)


# ---- build ---------------------------------------------------------------------------------------------------------------------------
def test_visloc_resource_report_has_no_scratch():
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'visloc.resources.txt')
    assert os.path.exists(path), 'built by dust3r_amd/build.py'
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    assert sum('match_' in k for k in kernels) == 3 and sum('pnp_' in k for k in kernels) == 10
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
    assert {'d3r_match_pairs', 'd3r_match_pairs_workspace', 'd3r_pnp_ransac', 'd3r_pnp_ransac_workspace'} <= set(_lib.EXPORTED)
    assert C.sizeof(_lib.MatchJob) == 56 and C.sizeof(_lib.PnpRansacJob) == 64
