"""CPU tests (-m "not gpu") of the visual-localization package: dust3r_amd.visloc.evaluation against restatements written here with
SciPy's Rotation, the binding of the reference's visloc.py imports through the INTEGRATION.md aliases, the host build of the shared
P3P / stopping-rule math of csrc/visloc.hip, OpenCV's undistortion loop, the homogeneous geotrf, and the kernels' resource report."""
import ctypes as C
import functools
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


# ---- d3r_pnp_ransac restated round by round -------------------------------------------------------------------------------------------
# What tests/test_visloc_ransac_gpu.py compares the ten pnp_* kernels of csrc/visloc.hip with, through the C ABI; the cases of that file
# are listed here so that test_every_gpu_case_is_unambiguous can vet them without a GPU.
from test_cloud_global_cpu import restated_samples  # noqa: E402

F32 = np.float32
FX, FY, CX, CY = 520.0, 480.0, 300.5, 210.25                      # every entry an fp32 number: the job record holds them as float
K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])
IMG_W, IMG_H = 640, 480
RND, MODEL_POINTS, CHUNK = 128, 4, 1024                           # csrc/visloc.hip
DELTA = 1e-3                                                      # the relative half-width of the gate's band (restated_pnp_ransac)
BIG_SEED = 2 ** 63 + 5


def pnp_problem(n, outliers, noise, seed):
    from dust3r_amd.synthetic import pnp_problem as make
    return make(n, outliers, noise, seed, K=K, size=(IMG_W, IMG_H))


def _camera(pose, X):
    """camera-frame points (..., n, 3) of fp64 poses (..., 3, 4); rows that are not finite give NaN quietly"""
    with np.errstate(invalid='ignore', over='ignore'):
        return np.einsum('...rc,nc->...nr', pose[..., :3], X) + pose[..., None, :, 3]


def gate_sets(pose, uv, X, thr, delta=DELTA):
    """(lo, hi) boolean (..., n): the rows in front of the camera of the fp64 pose(s) (..., 3, 4) whose pixel error, all in fp64 from the fp32
    rows, is <= thr (1 - delta) and <= thr (1 + delta). A row with a non-finite entry is in neither."""
    uv, X = np.asarray(uv, F32).astype(np.float64), np.asarray(X, F32).astype(np.float64)
    finite = np.isfinite(uv).all(axis=1) & np.isfinite(X).all(axis=1)
    uv, X = np.where(finite[:, None], uv, 0.0), np.where(finite[:, None], X, 0.0)
    Y = _camera(np.asarray(pose, np.float64), X)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        err = np.hypot(FX * Y[..., 0] / Y[..., 2] + CX - uv[:, 0], FY * Y[..., 1] / Y[..., 2] + CY - uv[:, 1])
        front = finite & (Y[..., 2] > 0)
        return front & (err <= thr * (1 - delta)), front & (err <= thr * (1 + delta))


def kernel_gate_f32(pose, uv, X, thr, finite_gate=True):
    """is_inlier of csrc/visloc.hip in numpy fp32, every operation rounded on its own: boolean (H, n) for fp64 poses (H, 3, 4).
    finite_gate=False: without its `thr^2 z^2 is finite` term, the expression that let inf <= inf through."""
    uv, X, pose = np.asarray(uv, F32), np.asarray(X, F32), np.asarray(pose, np.float64)
    rows = np.concatenate([(float(F32(FX)) * pose[:, 0]), (float(F32(FY)) * pose[:, 1]), pose[:, 2]], axis=1).astype(F32)[:, :, None]
    a, b = uv[:, 0] - F32(CX), uv[:, 1] - F32(CY)
    thr2 = F32(thr) * F32(thr)
    with np.errstate(invalid='ignore', over='ignore'):
        x = rows[:, 0] * X[:, 0] + rows[:, 1] * X[:, 1] + rows[:, 2] * X[:, 2] + rows[:, 3]
        y = rows[:, 4] * X[:, 0] + rows[:, 5] * X[:, 1] + rows[:, 6] * X[:, 2] + rows[:, 7]
        z = rows[:, 8] * X[:, 0] + rows[:, 9] * X[:, 1] + rows[:, 10] * X[:, 2] + rows[:, 11]
        ex, ey = x - a * z, y - b * z
        lim = thr2 * (z * z)
        assert x.dtype == F32 and lim.dtype == F32
        return (z > 0) & ((lim < np.inf) | (not finite_gate)) & (ex * ex + ey * ey <= lim)


def restated_pnp_hypotheses(uv, X, seed, hs):
    """(poses (H, 3, 4) float64, valid (H,), trusted (H,)) of the hypotheses `hs`: the sampler's four rows widened to fp64 through the host
    build of the solver (p3p_pick, pinned by test_p3p_*_host). No pose is trusted unchecked: it must be a rotation to 1e-8, put its three
    sample points on their pixels to 1e-6 px and all four in front of the camera (a near-degenerate sample's pose can miss that; the device's
    libm may then give a visibly different one, so such a pose must not win a round)."""
    uv64, X64 = np.asarray(uv, F32).astype(np.float64), np.asarray(X, F32).astype(np.float64)
    pick = restated_samples(seed, hs, len(uv64), k=MODEL_POINTS)
    poses, valid = np.zeros((len(pick), 12)), np.zeros(len(pick), bool)
    solve, pose = _lib.lib.d3r_selftest_p3p_host, np.zeros(12)
    for i, idx in enumerate(pick):
        if idx[MODEL_POINTS - 1] < 0:
            continue
        if solve(_dp(np.ascontiguousarray(uv64[idx])), _dp(np.ascontiguousarray(X64[idx])), float(F32(FX)), float(F32(FY)), float(F32(CX)),
                 float(F32(CY)), _dp(pose)) == 1:
            poses[i], valid[i] = pose, True
    poses = poses.reshape(-1, 3, 4)
    trusted = np.zeros(len(pick), bool)
    P, s = poses[valid], pick[valid]
    if len(P):
        R = P[:, :, :3]
        rotation = (np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)) < 1e-8) & (np.abs(np.linalg.det(R) - 1) < 1e-8)
        Y = np.einsum('hrc,hkc->hkr', R, X64[s]) + P[:, None, :, 3]
        pix = np.stack([FX * Y[..., 0] / Y[..., 2] + CX, FY * Y[..., 1] / Y[..., 2] + CY], axis=-1)
        trusted[valid] = rotation & (Y[..., 2] > 0).all(axis=1) & (np.abs(pix - uv64[s])[:, :3].max(axis=(1, 2)) < 1e-6)
    return poses, valid, trusted


def _first_best(counts, valid):
    """(index, count) of the largest count among the valid, the lowest index among equals; (-1, -1) without a valid one"""
    c = np.where(valid, counts, -1)
    k = int(np.argmax(c)) if len(c) else 0
    return (k, int(c[k])) if len(c) and c[k] >= 0 else (-1, -1)


def restated_pnp_ransac(uv, X, thr=5.0, confidence=0.9999, seed=0, max_iters=10_000, max_points=None, delta=DELTA):
    """d3r_pnp_ransac up to its polish, after the header comment of csrc/visloc.hip. Rounds of 128 hypotheses h < budget: restated_samples,
    restated_pnp_hypotheses, then every valid hypothesis's support three times: in fp64 under the gates thr (1 - delta) (`lo`) and
    thr (1 + delta) (`hi`) of gate_sets, and by kernel_gate_f32. The round's winner (largest support, then lowest index) replaces the best
    when its support is > max(best support, 3); the budget becomes RANSACUpdateNumIters(float32(confidence), (n - support) / n, 4, budget);
    the job is done when (round + 1) 128 >= budget; `drawn` adds min(128, budget at the round's start - 128 round). Status 1 when the best
    support is > 4. n <= 4, max_iters <= 0 and n > max_points: (0, 0, 0, -1), nothing drawn.

    Why a band and not bit equality: visloc.hip is compiled with FMA contraction and the device's fp64 libm differs from the host's in the
    last bits of a pose, so the kernel's fp32 test can differ from any host evaluation for a point AT the gate. delta = 1e-3 is derived: the
    fp32 products of is_inlier reach about 2000-5000 px x depth, half an ulp there is <= 3e-4, over the four terms of a row at a depth >= 2
    that stays below 1.5e-4 px, which is 1.5e-4 of thr = 1 and 3e-5 of thr = 5: the band leaves a factor >= 6. The result is `unambiguous`
    when in every round the winner is the same under lo, hi and the fp32 evaluation with three equal supports (so the best hypothesis's lo
    and hi sets are equal) and its pose passed restated_pnp_hypotheses' check: no point within the band then decides anything, and
    (status, drawn, best_h) must be the kernel's exactly.

    Returns dict(status, best_h, best_support, drawn, pose (3, 4) or None, lo, hi (n,) bool, unambiguous, rounds)."""
    uv, X = np.asarray(uv, F32).reshape(-1, 2), np.asarray(X, F32).reshape(-1, 3)
    n = len(uv)
    out = dict(status=0, best_h=-1, best_support=0, drawn=0, pose=None, lo=np.zeros(n, bool), hi=np.zeros(n, bool), unambiguous=True, rounds=0)
    if n <= MODEL_POINTS or max_iters <= 0 or (max_points is not None and n > max_points):
        return out
    budget, r = int(max_iters), 0
    while True:
        hs = np.arange(r * RND, min((r + 1) * RND, budget))
        out['drawn'] += len(hs)
        poses, valid, trusted = restated_pnp_hypotheses(uv, X, seed, hs)
        lo, hi = gate_sets(poses, uv, X, thr, delta)
        f32 = kernel_gate_f32(poses, uv, X, thr)
        wins = [_first_best(s.sum(axis=1), valid) for s in (lo, hi, f32)]
        bl, bc = wins[2]
        out['unambiguous'] &= wins[0] == wins[1] == wins[2] and (bl < 0 or bool(trusted[bl]))
        if bl >= 0 and bc > max(out['best_support'], MODEL_POINTS - 1):
            out.update(best_support=bc, best_h=int(hs[bl]), pose=poses[bl], lo=lo[bl], hi=hi[bl])
            out['unambiguous'] &= bool(np.array_equal(lo[bl], hi[bl]))
            budget = _update_num_iters(float(F32(confidence)), (n - bc) / n, MODEL_POINTS, budget)
        r += 1
        if r * RND >= budget:
            break
    out.update(status=int(out['best_support'] > MODEL_POINTS), rounds=r)
    return out


def pnp_abi(jobs, gpu, max_iters=10_000, params=None):
    """d3r_pnp_ransac straight through the C ABI (no Python-side n <= 4 shortcut). A job is (uv, X) or a dict(uv, X[, thr, confidence, seed,
    max_iters, inlier_mask]); params: (max_iters, max_points) of the call, by default the largest of the jobs. Returns
    ([(status, inliers, drawn, best index)], poses (m, 3, 4) float64, [mask uint8 (n,) or None]); a mask starts as all 7."""
    from dust3r_amd._lib import PnpRansacJob, PnpRansacParams, check, current_stream, lib, ptr
    from dust3r_amd.visloc.localization import _records
    keep, recs, masks = [], [], []
    for job in jobs:
        job = dict(uv=job[0], X=job[1]) if isinstance(job, tuple) else job
        p2 = torch.as_tensor(job['uv'], dtype=torch.float32, device=gpu).reshape(-1, 2).contiguous()
        p3 = torch.as_tensor(job['X'], dtype=torch.float32, device=gpu).reshape(-1, 3).contiguous()
        mask = torch.full((len(p2),), 7, dtype=torch.uint8, device=gpu) if job.get('inlier_mask', False) else None
        keep += [p2, p3]
        masks.append(mask)
        recs.append(PnpRansacJob(p2.data_ptr(), p3.data_ptr(), None if mask is None else mask.data_ptr(), len(p2), job.get('max_iters', max_iters),
                                 FX, FY, CX, CY, job.get('thr', 5.0), job.get('confidence', 0.9999), job.get('seed', 0)))
    m = len(recs)
    params = PnpRansacParams(*(params or (max(max(r.max_iters for r in recs), 0), max(max(r.n for r in recs), 1))))
    rec = _records(recs, PnpRansacJob, gpu)
    work = torch.empty(int(lib.d3r_pnp_ransac_workspace(m, params.max_points)), dtype=torch.uint8, device=gpu)
    poses = torch.empty((m, 12), dtype=torch.float64, device=gpu)
    inl, status, stats = (torch.empty(s, dtype=torch.int32, device=gpu) for s in (m, m, (m, 2)))
    check(lib.d3r_pnp_ransac(m, ptr(rec), C.byref(params), ptr(work), ptr(poses), ptr(inl), ptr(status), ptr(stats), current_stream()), 'pnp')
    out = [(int(a), int(b), int(c), int(d)) for a, b, (c, d) in zip(status.cpu(), inl.cpu(), stats.cpu().tolist())]
    return out, poses.cpu().numpy().reshape(m, 3, 4), [None if k is None else k.cpu().numpy() for k in masks]


# ---- the cases of tests/test_visloc_ransac_gpu.py ----------------------------------------------------------------------------------------
def _case(name, uv, X, thr=5.0, seed=0, max_iters=10_000, **extra):
    return dict(name=name, uv=uv, X=X, thr=thr, confidence=0.9999, seed=seed, max_iters=max_iters, inlier_mask=True, **extra)


def restated(case, max_points=None):
    """restated_pnp_ransac of a case, computed once"""
    key = ('want', max_points)
    if key not in case:
        case[key] = restated_pnp_ransac(case['uv'], case['X'], case['thr'], case['confidence'], case['seed'], case['max_iters'], max_points)
    return case[key]


ROUND_NS = (5, 6, 7, 64, 1023, 1024, 1025, 2049)                  # 5: the smallest n that runs; 1024: a scoring workgroup's points
# the two cases of the matrix with a point inside the band under their listed seed (found on the CPU) run under another one
RESEEDED = {(2049, 0.6, 0.5, 1, 5.0): 3, (64, 0.3, 0.5, BIG_SEED, 1.0): BIG_SEED + 1}


@functools.lru_cache(maxsize=None)
def round_cases(n):
    cases = []
    for thr in (5.0, 1.0) if n <= 64 else (5.0,):                # thr = 1 above 64 points: about one planted inlier per hypothesis in the band
        for o in (0.0, 0.3, 0.6):
            for s in (0.0, 0.5):
                uv, X, w2c, inl = pnp_problem(n, o, s, n + int(10 * o) + int(100 * s))
                for seed in (0, 1, BIG_SEED):
                    seed = RESEEDED.get((n, o, s, seed, thr), seed)
                    cases.append(_case(f'n{n} o{o} s{s} seed{seed} thr{thr}', uv, X, thr, seed, 300 if n <= 7 else 10_000, w2c=w2c, planted=inl))
    return cases


@functools.lru_cache(maxsize=None)
def budget_cases():
    uv, X, _, _ = pnp_problem(300, 0.6, 0.5, 356)
    return [_case(f'budget {m}', uv, X, max_iters=m) for m in (1, 127, 128, 129, 300)]


def mirrored_problem(n):
    """pnp_problem(n, 0, 0, 77 + n) with every third point mirrored through the camera centre, X' = R^T (-(R X + t) - t): the same pixel
    (recomputed from the fp32 X' by the same projective formula), behind the camera. Returns (uv, X, w2c, mirrored)."""
    uv, X, w2c, _ = pnp_problem(n, 0.0, 0.0, 77 + n)
    R, t = w2c[:3, :3], w2c[:3, 3]
    mirrored = np.arange(n) % 3 == 0
    Xm = ((-(X.astype(np.float64) @ R.T + t) - t) @ R).astype(F32)
    pix, z = _project(w2c, Xm.astype(np.float64), FX, FY, CX, CY)
    assert (z[mirrored] < -2).all() and np.abs(pix - uv)[mirrored].max() < 1e-3
    return np.where(mirrored[:, None], pix.astype(F32), uv), np.where(mirrored[:, None], Xm, X), w2c, mirrored


@functools.lru_cache(maxsize=None)
def cheirality_cases():
    cases = []
    for n in (600, 1025):
        uv, X, w2c, mirrored = mirrored_problem(n)
        cases += [_case(f'mirrored n{n} seed{seed}', uv, X, seed=seed, w2c=w2c, mirrored=mirrored) for seed in (0, 1, BIG_SEED)]
    return cases


NON_FINITE = [('X', 0, -np.inf), ('X', 1, np.inf), ('X', 2, -np.inf), ('X', slice(None), np.inf), ('X', 1, np.nan), ('uv', 0, np.nan),
              ('uv', 1, np.inf), ('X', 0, np.inf), ('X', 1, -np.inf), ('X', 2, np.inf), ('X', slice(None), -np.inf), ('uv', 0, -np.inf)]


@functools.lru_cache(maxsize=None)
def non_finite_cases():
    """noiseless problems with every `step`-th row from row 1 spoilt, the kinds of NON_FINITE in turn (row 1 of the 64-point problem of
    seed 0 with X[1, 0] = -inf is a row that the kernel's fp32 expression alone lets through at the true pose)"""
    cases = []
    for n, step in ((64, 9), (1025, 10)):
        uv, X, w2c, _ = pnp_problem(n, 0.0, 0.0, 0)
        arrays = dict(uv=uv.copy(), X=X.copy())
        bad = np.arange(1, n, step)
        for k, row in enumerate(bad):
            which, col, value = NON_FINITE[k % len(NON_FINITE)]
            arrays[which][row, col] = value
        spoilt = np.zeros(n, bool)
        spoilt[bad] = True
        cases += [_case(f'non-finite n{n} seed{seed}', arrays['uv'], arrays['X'], seed=seed, w2c=w2c, spoilt=spoilt) for seed in (0, BIG_SEED)]
    return cases


def _pure_outliers(n, seed):
    rng = np.random.RandomState(seed)
    return np.c_[rng.uniform(0, IMG_W, n), rng.uniform(0, IMG_H, n)].astype(F32), (rng.normal(size=(n, 3)) + [0, 0, 5]).astype(F32)


MANY_JOBS = (64, 65, 130)


@functools.lru_cache(maxsize=None)
def many_jobs(n_jobs):
    """n_jobs mixed jobs (job k is the same in every list) with failing ones at 0, 63, 64 and the last: n = 4 and pure outliers in turn"""
    cases = []
    for k in range(n_jobs):
        rng = np.random.RandomState(1000 + k)
        n, o, s = int(rng.choice([5, 6, 9, 17, 64, 150, 300])), float(rng.choice([0.0, 0.3, 0.6])), float(rng.choice([0.0, 0.5]))
        thr, seed = float(rng.choice([3.0, 5.0])), [k, 2 ** 32 + k, 2 ** 63 + k][rng.randint(3)]
        seed = 2 ** 32 + 1098 if k == 98 else seed             # job 98 has a point inside the band under 2^32 + 98 (found on the CPU)
        uv, X, _, _ = pnp_problem(n, o, s, 500 + k)
        cases.append(_case(f'job {k}: n{n} o{o} s{s} thr{thr} seed{seed}', uv, X, thr, seed, 300))
    for i, k in enumerate(sorted({0, 63, 64, n_jobs - 1} & set(range(n_jobs)))):
        uv, X = (cases[k]['uv'][:4], cases[k]['X'][:4]) if i % 2 == 0 else _pure_outliers(30, 2000 + k)
        cases[k] = _case(f'job {k}: failing, n{len(uv)}', uv, X, cases[k]['thr'], cases[k]['seed'], 300, fails=True)
    return cases


@functools.lru_cache(maxsize=None)
def lm_case():
    """noise 0.5 against thr = 1: the best hypothesis, solved from noisy samples, is supported by a strict subset of the planted set"""
    uv, X, w2c, inl = pnp_problem(64, 0.0, 0.5, 114)
    return _case('lm set', uv, X, 1.0, 0, w2c=w2c, planted=inl)


@functools.lru_cache(maxsize=None)
def seed_cases():
    """two seeds with the same lower 32 bits, under run_pnp_batch's settings"""
    uv, X, _, _ = pnp_problem(300, 0.6, 0.5, 356)
    return [_case(f'seed {seed}', uv, X, seed=seed) for seed in (BIG_SEED, BIG_SEED - 2 ** 63)]


def every_gpu_case():
    return ([c for n in ROUND_NS for c in round_cases(n)] + budget_cases() + cheirality_cases() + non_finite_cases()
            + [c for m in MANY_JOBS for c in many_jobs(m)] + [lm_case()] + seed_cases())


# ---- the restatement's own tests ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [5, 64, 1025])
def test_restated_pnp_on_noiseless_problems(n):
    uv, X, w2c, _ = pnp_problem(n, 0.0, 0.0, 7 + n)
    for seed in (0, BIG_SEED):
        _, valid, _ = restated_pnp_hypotheses(uv, X, seed, np.arange(RND))
        want = restated_pnp_ransac(uv, X, seed=seed)
        assert (want['status'], want['best_support'], want['drawn'], want['unambiguous']) == (1, n, RND, True)
        assert want['best_h'] == np.flatnonzero(valid)[0] and want['lo'].all()
        assert np.abs(want['pose'] - w2c[:3]).max() < 1e-5


@pytest.mark.parametrize('outliers,noise', [(0.3, 0.0), (0.6, 0.0), (0.3, 0.5), (0.6, 0.5)])
def test_restated_pnp_with_outliers_finds_the_planted_set(outliers, noise):
    uv, X, _, inl = pnp_problem(1024, outliers, noise, 31)
    want = restated_pnp_ransac(uv, X)
    assert want['status'] == 1 and want['unambiguous'] and np.array_equal(want['lo'], inl) and np.array_equal(want['hi'], inl)
    assert want['best_support'] == inl.sum() and (want['rounds'] - 1) * RND < want['drawn'] <= want['rounds'] * RND < 1024


def test_restated_pnp_support_of_the_sample_alone():
    """6 points, 2 of them outliers: the best any hypothesis gets is its own 4 points. That sets best_h and shrinks the budget to
    RANSACUpdateNumIters(0.9999, 2 / 6, 4) = 42 <= 128, so the job ends after one round -- and fails, as 4 is not more than the sample."""
    uv, X, _, inl = pnp_problem(6, 0.3, 0.0, 3)
    assert inl.sum() == 4 and _update_num_iters(float(F32(0.9999)), 2 / 6, 4, 300) == 42
    want = restated_pnp_ransac(uv, X, max_iters=300)
    assert (want['status'], want['best_support'], want['drawn']) == (0, 4, RND) and want['best_h'] >= 0 and want['unambiguous']
    assert np.array_equal(want['lo'], inl)


def test_restated_pnp_jobs_that_do_not_run():
    uv, X, _, _ = pnp_problem(8, 0.0, 0.0, 1)
    for want in (restated_pnp_ransac(uv[:4], X[:4]), restated_pnp_ransac(uv, X, max_iters=0), restated_pnp_ransac(uv, X, max_points=7)):
        assert (want['status'], want['best_support'], want['drawn'], want['best_h']) == (0, 0, 0, -1) and want['pose'] is None


def test_restated_pnp_budget_below_a_round():
    uv, X, _, _ = pnp_problem(300, 0.6, 0.5, 356)
    assert [restated_pnp_ransac(uv, X, max_iters=m)['drawn'] for m in (1, 127, 128, 129)] == [1, 127, 128, 129]


def test_every_gpu_case_is_unambiguous():
    """every case that tests/test_visloc_ransac_gpu.py compares exactly: no point within the band decides a round of its restatement"""
    cases = every_gpu_case()
    assert len(cases) == 144 + 72 + 5 + 6 + 4 + sum(MANY_JOBS) + 1 + 2
    bad = [c['name'] for c in cases if not restated(c)['unambiguous']]
    assert not bad, bad
    for c in cheirality_cases():
        assert restated(c)['drawn'] == RND and not restated(c)['lo'][c['mirrored']].any()
    for c in non_finite_cases():
        # the rows the old expression let through at the true pose are there, or the GPU test could not see it
        through = kernel_gate_f32(c['w2c'][None, :3], c['uv'], c['X'], 5.0, finite_gate=False)[0] & c['spoilt']
        assert through.any() and (c['name'] != 'non-finite n64 seed0' or through[1])
        assert not kernel_gate_f32(c['w2c'][None, :3], c['uv'], c['X'], 5.0)[0][c['spoilt']].any()
    want = restated(lm_case())
    assert want['status'] == 1 and (want['lo'] <= lm_case()['planted']).all() and want['best_support'] < lm_case()['planted'].sum()
