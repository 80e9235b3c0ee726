"""Cloud registration (Sim(3) ICP) without a GPU: the numpy restatements that tests/test_cloud_icp_gpu.py holds csrc/cloud_icp.hip and
cloud_metrics.register_clouds against, pinned here against the truth on a synthetic scene, and the host algebra of the update.
- `restated_transform`: float32, row r = ((A_r0 x + A_r1 y) + A_r2 z) + t_r, every numpy operation one fp32 rounding: bit-exact by
  construction.
- `restated_used_and_sums`: the gates of d3r_cloud_icp_sums (include/dust3r_hip.h) and, per used row, the fp64 terms in the header's
  operation order; the sums are numpy's fp64 sums of those terms.
- `restated_register`: the loop of register_clouds with cKDTree as the nearest neighbour, the same gates and stop rule, and an update
  that does not go through the sums: least squares on the stacked rows J x = -e (plane), Umeyama on the pairs (point).
The scene: a bumpy ellipsoid without symmetry, reference 6000 points with PCA normals (k = 12), source 5000 fresh samples (or a subset of
the reference) plus 250 uniform outliers, moved by the inverse of a known similarity (8 degrees about (1, 2, 3), scale 1.08)."""
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree

from dust3r_amd.cloud_metrics import Registration, icp_update, plane_system, register_clouds, similarity_parts      # what this file is about
from test_cloud_metrics_cpu import valid_rows

F32 = np.float32
STAGES = (0.3, 0.1, 0.03)
MAX_ITERS = 30


# ---- restatements ------------------------------------------------------------------------------------------------------------------------
def restated_transform(P, M, normals=None, R=None):
    """P (n, 3) float32 moved by M (12,) float32 = [A | t] row-major; normals rotated by R (9,) float32. float32 throughout."""
    P, M = np.asarray(P, F32), np.asarray(M, F32).reshape(3, 4)
    with np.errstate(invalid='ignore', over='ignore'):
        x, y, z = P[:, 0], P[:, 1], P[:, 2]
        out = np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], axis=1)
        assert out.dtype == F32
        if normals is None:
            return out
        N, R = np.asarray(normals, F32), np.asarray(R, F32).reshape(3, 3)
        x, y, z = N[:, 0], N[:, 1], N[:, 2]
        rot = np.stack([(R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z for r in range(3)], axis=1)
    assert rot.dtype == F32
    return out, rot


def restated_used_and_sums(moved, ref, d2, idx, metric, gate, centre, ref_normals=None, moved_normals=None, cos_min=None):
    """(used (n,) bool, count, sums (18 or 36,) float64, terms (count, 18 or 36) float64): the definition of d3r_cloud_icp_sums. sums =
    terms.sum(axis=0) in numpy's order; the kernel adds the same doubles in another order."""
    moved, ref = np.asarray(moved, F32), np.asarray(ref, F32)
    idx, d2 = np.asarray(idx, np.int64), np.asarray(d2, F32)
    gate = F32(gate)
    with np.errstate(invalid='ignore', over='ignore'):
        used = (idx >= 0) & (idx < len(ref)) & (d2 <= gate * gate) & valid_rows(moved)
        g = np.where(used, idx, 0)
        used &= valid_rows(ref[g])
        if metric == 'plane':
            n32 = np.asarray(ref_normals, F32)[g]
            used &= valid_rows(n32) & (n32 != 0).any(axis=1)
        if moved_normals is not None:
            m, n32 = np.asarray(moved_normals, F32), np.asarray(ref_normals, F32)[g]
            cos = (m[:, 0] * n32[:, 0] + m[:, 1] * n32[:, 1]) + m[:, 2] * n32[:, 2]
            assert cos.dtype == F32
            used &= cos >= F32(cos_min)
    c = np.asarray(centre, F32).astype(np.float64)
    a = moved[used].astype(np.float64) - c
    y = ref[g[used]].astype(np.float64) - c
    d = a - y
    dot = lambda u, v: (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]      # noqa: E731
    if metric == 'point':
        cols = [np.ones(len(a))] + [a[:, i] for i in range(3)] + [y[:, i] for i in range(3)]
        cols += [a[:, i] * y[:, j] for i in range(3) for j in range(3)] + [dot(a, a), dot(d, d)]
    else:
        n = np.asarray(ref_normals, F32)[g[used]].astype(np.float64)
        J = [a[:, 1] * n[:, 2] - a[:, 2] * n[:, 1], a[:, 2] * n[:, 0] - a[:, 0] * n[:, 2], a[:, 0] * n[:, 1] - a[:, 1] * n[:, 0],
             n[:, 0], n[:, 1], n[:, 2], dot(a, n)]
        e = dot(n, d)
        cols = [J[r] * J[k] for r in range(7) for k in range(r, 7)] + [J[r] * e for r in range(7)] + [e * e]
    terms = np.stack(cols, axis=1) if len(a) else np.zeros((0, len(cols)))
    return used, int(used.sum()), terms.sum(axis=0), terms


def exp_so3(w):
    t = np.linalg.norm(w)
    if t == 0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


def similarity(axis, degrees, scale, t):
    axis = np.asarray(axis, np.float64)
    S = np.eye(4)
    S[:3, :3] = scale * exp_so3(axis / np.linalg.norm(axis) * math.radians(degrees))
    S[:3, 3] = t
    return S


def similarity_distance(S, T):
    """(rotation angle in degrees, |s_S / s_T - 1|, |t_S - t_T|) between two similarities"""
    sS, sT = np.cbrt(np.linalg.det(S[:3, :3])), np.cbrt(np.linalg.det(T[:3, :3]))
    chord = np.linalg.norm(S[:3, :3] / sS - T[:3, :3] / sT) / (2 * math.sqrt(2))
    return math.degrees(2 * math.asin(min(chord, 1.0))), abs(sS / sT - 1), float(np.linalg.norm(S[:3, 3] - T[:3, 3]))


def nearest_by_tree(tree, ref, moved, gate):
    """(d2 float32, idx) with cKDTree choosing the neighbour and the kernels' fp32 expression giving d2; -1 / inf beyond the gate or for
    a non-finite point"""
    ok = valid_rows(moved)
    idx = np.full(len(moved), -1, np.int64)
    d2 = np.full(len(moved), np.inf, F32)
    _, j = tree.query(moved[ok].astype(np.float64), k=1, distance_upper_bound=float(gate) * 1.001)
    found = j < len(ref)
    rows = np.flatnonzero(ok)[found]
    dd = moved[rows] - ref[j[found]]
    m = dd * dd
    v = (m[:, 0] + m[:, 1]) + m[:, 2]
    keep = v <= F32(gate) * F32(gate)
    idx[rows[keep]], d2[rows[keep]] = j[found][keep], v[keep]
    return d2, idx


def restated_update(metric, a, y, n, with_scale):
    """(A (3, 3), v (3,)) of the map a -> A a + v that the iteration applies about the centre, straight from the pairs"""
    if metric == 'point':
        ma, my = a.mean(axis=0), y.mean(axis=0)
        U, sv, Vt = np.linalg.svd((y - my).T @ (a - ma) / len(a))
        dd = np.array([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
        R = (U * dd) @ Vt
        s = (sv * dd).sum() / ((a - ma) ** 2).sum(axis=1).mean() if with_scale else 1.0
        return s * R, my - s * R @ ma
    J = np.concatenate([np.cross(a, n), n, (a * n).sum(axis=1, keepdims=True)], axis=1)[:, :7 if with_scale else 6]
    e = (n * (a - y)).sum(axis=1)
    x = np.linalg.lstsq(J, -e, rcond=None)[0]
    return (math.exp(x[6]) if with_scale else 1.0) * exp_so3(x[:3]), x[3:6]


def restated_register(src, dst, dst_normals, stages, init=None, with_scale=True, metric='plane', max_iters=MAX_ITERS, tol=1e-6, centre=None):
    """(S, history [(stage, n_pairs, rmse)], converged): the loop of register_clouds"""
    src, dst = np.asarray(src, F32), np.asarray(dst, F32)
    S = np.eye(4) if init is None else np.array(init, np.float64)
    ok = valid_rows(dst)
    c = ((dst[ok].min(axis=0).astype(np.float64) + dst[ok].max(axis=0).astype(np.float64)) * 0.5).astype(F32) if centre is None else np.asarray(centre, F32)
    c64 = c.astype(np.float64)
    tree = cKDTree(dst.astype(np.float64))
    history, converged = [], False
    for stage, gate in enumerate(stages):
        prev, converged = None, False
        for _ in range(max_iters):
            moved = restated_transform(src, S[:3, :4].astype(F32).reshape(12))
            d2, idx = nearest_by_tree(tree, dst, moved, gate)
            used, count, sums, _ = restated_used_and_sums(moved, dst, d2, idx, metric, gate, c, ref_normals=dst_normals)
            rmse = math.sqrt(sums[17 if metric == 'point' else 35] / count)
            history.append((stage, count, rmse))
            if prev is not None and abs(rmse - prev) <= tol * rmse:
                converged = True
                break
            prev = rmse
            a, y = moved[used].astype(np.float64) - c64, dst[idx[used]].astype(np.float64) - c64
            n = None if metric == 'point' else np.asarray(dst_normals, F32)[idx[used]].astype(np.float64)
            A, v = restated_update(metric, a, y, n, with_scale)
            D = np.eye(4)
            D[:3, :3], D[:3, 3] = A, c64 + v - A @ c64
            S = D @ S
    return S, history, converged


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------
TRUTH = similarity((1, 2, 3), 8.0, 1.08, (0.05, -0.03, 0.04))


def ellipsoid(rng, n):
    """n points u r(u) (1, 0.8, 0.6), r = 1 + 0.15 sin(3 u_x + 1) cos(2 u_y) + 0.1 u_z^3, u uniform on the sphere"""
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 1 + 0.15 * np.sin(3 * u[:, 0] + 1) * np.cos(2 * u[:, 1]) + 0.1 * u[:, 2] ** 3
    return (u * r[:, None] * np.array([1.0, 0.8, 0.6])).astype(F32)


def pca_normals(P, k=12):
    P64 = P.astype(np.float64)
    _, nbr = cKDTree(P64).query(P64, k=k + 1)
    Q = P64[nbr]
    Q = Q - Q.mean(axis=1, keepdims=True)
    _, vec = np.linalg.eigh(np.einsum('nki,nkj->nij', Q, Q))
    return vec[:, :, 0].astype(F32)


_SCENES = {}


def scene(kind):
    """(src, dst, dst_normals) float32: kind 'fresh' = 5000 fresh samples, 'subset' = 5000 points of the reference; both with 250 uniform
    outliers in [-1.5, 1.5]^3 behind them, moved by the inverse of TRUTH. Built once."""
    if kind not in _SCENES:
        rng = np.random.default_rng(20240611)
        dst = ellipsoid(rng, 6000)
        normals = pca_normals(dst)
        clean = ellipsoid(rng, 5000) if kind == 'fresh' else dst[rng.permutation(len(dst))[:5000]]
        pts = np.concatenate([clean.astype(np.float64), rng.uniform(-1.5, 1.5, (250, 3))])
        inv = np.linalg.inv(TRUTH)
        _SCENES[kind] = ((pts @ inv[:3, :3].T + inv[:3, 3]).astype(F32), dst, normals)
    return _SCENES[kind]


RIGID_INIT = np.diag([1.08, 1.08, 1.08, 1.0])      # the rigid runs start at the true scale and keep it

# (kind, metric, with_scale) -> the bars of the restatement against the truth: (degrees, relative scale, translation), twice what a
# prototype of the restatement reached
CASES = {('fresh', 'plane', True): (0.03, 4.4e-4, 1e-4), ('fresh', 'plane', False): (0.03, 4.4e-4, 1e-4),
         ('subset', 'plane', True): (0.022, 2e-5, 4.6e-5), ('subset', 'plane', False): (0.022, 2e-5, 4.6e-5),
         ('subset', 'point', True): (1.2e-3, 2e-5, None)}
_RESTATED = {}


def restated_case(kind, metric, with_scale):
    """(S, history, converged) of the restatement on a case, computed once and shared with the GPU tests"""
    key = (kind, metric, with_scale)
    if key not in _RESTATED:
        src, dst, normals = scene(kind)
        _RESTATED[key] = restated_register(src, dst, normals, STAGES, init=None if with_scale else RIGID_INIT, with_scale=with_scale, metric=metric)
    return _RESTATED[key]


def stage_counts(history, n_stages=len(STAGES)):
    return [sum(1 for h in history if h[0] == s) for s in range(n_stages)]


# ---- 1. the restatement against the truth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,metric,with_scale', list(CASES))
def test_restatement_recovers_the_truth(kind, metric, with_scale):
    S, history, converged = restated_case(kind, metric, with_scale)
    ang, ds, dt = similarity_distance(S, TRUTH)
    print(f'{kind} {metric} with_scale={with_scale}: {ang:.3g} deg, scale {ds:.3g}, translation {dt:.3g}, iterations {stage_counts(history)}')
    bar = CASES[kind, metric, with_scale]
    counts = stage_counts(history)
    assert converged and 1 < counts[-1] < MAX_ITERS, counts                            # the last stage met the tolerance before the cap
    if metric == 'plane':          # the plane metric converges in every stage, under 50 iterations in all; the point metric creeps
        assert all(1 < c < MAX_ITERS for c in counts) and sum(counts) < 50, counts     # tangentially and may spend a coarse stage's cap
    assert ang <= bar[0] and ds <= bar[1] and (bar[2] is None or dt <= bar[2])


def test_restated_transform_is_the_fp32_row_product():
    rng = np.random.default_rng(3)
    P = rng.standard_normal((200, 3)).astype(F32)
    M = TRUTH[:3, :4].astype(F32).reshape(12)
    got = restated_transform(P, M)
    want = P.astype(np.float64) @ TRUTH[:3, :3].T + TRUTH[:3, 3]
    assert got.dtype == F32 and np.abs(got - want).max() <= 4 * np.finfo(F32).eps * (np.abs(P) @ np.abs(TRUTH[:3, :3]).T + np.abs(TRUTH[:3, 3])).max()
    P[3, 1], P[5, 0] = np.nan, np.inf
    bad = restated_transform(P, M)
    assert not np.isfinite(bad[[3, 5]]).any() and np.isfinite(np.delete(bad, [3, 5], axis=0)).all()


# ---- 2. the host algebra -----------------------------------------------------------------------------------------------------------------
def _pairs(rng, D, n=400):
    """moved points a (about a centre), targets y = D applied, random unit normals; as the inputs of restated_used_and_sums"""
    c = np.array([0.3, -0.2, 0.1], F32)
    moved = (rng.standard_normal((n, 3)) + c).astype(F32)
    ref = (moved.astype(np.float64) @ D[:3, :3].T + D[:3, 3]).astype(F32)
    normals = rng.standard_normal((n, 3))
    normals = (normals / np.linalg.norm(normals, axis=1, keepdims=True)).astype(F32)
    d = moved - ref
    d2 = ((d * d)[:, 0] + (d * d)[:, 1]) + (d * d)[:, 2]
    return moved, ref, normals, d2, np.arange(n), c


@pytest.mark.parametrize('with_scale', [True, False])
@pytest.mark.parametrize('metric', ['point', 'plane'])
def test_update_from_hand_made_sums_reproduces_a_small_similarity(metric, with_scale):
    """targets y = D moved with D a rotation of 1e-4 rad (and scale 1 + 1e-4): the point update is Umeyama, exact to the fp32 rounding of
    the targets (6e-8 of coordinates of size 3); the plane update is one Gauss-Newton step, off by the second order, 1e-8"""
    D = similarity((2, -1, 0.5), math.degrees(1e-4), 1 + 1e-4 if with_scale else 1.0, (2e-4, -1e-4, 3e-4))
    moved, ref, normals, d2, idx, c = _pairs(np.random.default_rng(5), D)
    used, count, sums, _ = restated_used_and_sums(moved, ref, d2, idx, metric, 1.0, c, ref_normals=normals)
    assert count == len(moved)
    delta, rmse, reason = icp_update(metric, sums, count, c.astype(np.float64), with_scale)
    assert reason is None and np.abs(delta - D).max() <= 1e-6, np.abs(delta - D).max()
    assert rmse > 0 and (with_scale or abs(np.linalg.det(delta[:3, :3]) - 1) <= 1e-12)


def test_rigid_system_is_the_leading_6x6_block():
    sums = np.arange(1.0, 37.0)
    H7, g7, see = plane_system(sums, True)
    H6, g6, _ = plane_system(sums, False)
    assert H7.shape == (7, 7) and H6.shape == (6, 6) and np.array_equal(H7, H7.T) and see == 36.0
    assert np.array_equal(H7[0], sums[:7]) and H7[1, 1] == 8.0 and H7[6, 6] == 28.0 and np.array_equal(g7, sums[28:35])
    assert np.array_equal(H6, H7[:6, :6]) and np.array_equal(g6, g7[:6])


def test_singular_systems_report_a_reason_and_do_not_raise():
    rng = np.random.default_rng(6)
    moved, ref, normals, d2, idx, c = _pairs(rng, similarity((0, 0, 1), 0.01, 1.0, (1e-3, 0, 0)))
    flat = np.tile(np.array([[0, 0, 1]], F32), (len(moved), 1))                      # parallel planes fix one translation only
    _, count, sums, _ = restated_used_and_sums(moved, ref, d2, idx, 'plane', 1.0, c, ref_normals=flat)
    delta, rmse, reason = icp_update('plane', sums, count, c.astype(np.float64))
    assert delta is None and 'singular' in reason and rmse >= 0
    _, count, sums, _ = restated_used_and_sums(moved[:5], ref[:5], d2[:5], idx[:5], 'plane', 1.0, c, ref_normals=normals)
    assert icp_update('plane', sums, count, c.astype(np.float64))[2] == '5 pairs, 7 needed'
    line = np.outer(np.linspace(-1, 1, 50), [1, 2, 3]).astype(F32)                  # collinear points fix no rotation about the line
    _, count, sums, _ = restated_used_and_sums(line, line, np.zeros(50, F32), np.arange(50), 'point', 1.0, c)
    delta, _, reason = icp_update('point', sums, count, c.astype(np.float64))
    assert delta is None and 'singular' in reason
    assert icp_update('point', np.zeros(18), 0, c.astype(np.float64))[2] == '0 pairs, 3 needed'


def test_similarity_parts_and_the_transform_of_a_cloud():
    from dust3r_amd.viz import FusedCloud
    M, R, s = similarity_parts(TRUTH)
    assert M.dtype == F32 and R.dtype == F32 and abs(s - 1.08) <= 1e-12
    assert np.array_equal(M.reshape(3, 4), TRUTH[:3, :4].astype(F32)) and np.array_equal(R.reshape(3, 3), (TRUTH[:3, :3] / s).astype(F32))
    for bad in (np.eye(3), np.diag([1.0, 1.0, -1.0, 1.0]), np.diag([1.0, 2.0, 1.0, 1.0]), np.full((4, 4), np.nan), np.eye(4) + np.eye(4)[::-1] * 0.1):
        with pytest.raises(ValueError):
            similarity_parts(bad)
    empty = FusedCloud(np.zeros((0, 3), F32), np.zeros((0, 3), np.uint8), np.zeros(0, F32), np.zeros(0, np.int32), voxel_size=0.5,
                       bounds=(np.full(3, np.inf, F32), np.full(3, -np.inf, F32)))
    moved = empty.transform(TRUTH)                                                    # no point: nothing runs on a device
    assert len(moved) == 0 and moved.voxel_size == pytest.approx(0.54) and moved.normals is None
    with pytest.raises(ValueError):
        empty.transform(np.diag([1.0, 2.0, 1.0, 1.0]))
    assert Registration._fields == ('similarity', 'scale', 'rmse', 'n_pairs', 'n_valid', 'iterations', 'converged', 'reason', 'history')


def test_register_clouds_checks_its_arguments_before_the_device():
    P = np.zeros((4, 3), F32)
    for kw in (dict(metric='surface'), dict(max_dist=[]), dict(max_dist=-1.0), dict(max_iters=0), dict(init=np.diag([1.0, 2.0, 1.0, 1.0]))):
        with pytest.raises(ValueError):
            register_clouds(P, P, **dict(dict(max_dist=1.0), **kw))


def test_exports_refuse_bad_arguments_without_a_launch():
    import ctypes as C
    from dust3r_amd._lib import EXPORTED, lib
    assert {'d3r_cloud_transform', 'd3r_cloud_icp_sums', 'd3r_cloud_icp_sums_workspace_bytes'} <= set(EXPORTED)
    assert lib.d3r_cloud_icp_sums_workspace_bytes(0) == 0 and lib.d3r_cloud_icp_sums_workspace_bytes(1) >= 36 * 8 + 8
    assert lib.d3r_cloud_icp_sums_workspace_bytes(2 ** 31 - 1) == lib.d3r_cloud_icp_sums_workspace_bytes(1024 * 256)
    one = C.c_void_p(256)                                                             # never dereferenced: every call below is refused first
    M, R, c = (C.c_float * 12)(*np.eye(4)[:3].reshape(-1)), (C.c_float * 9)(*np.eye(3).reshape(-1)), (C.c_float * 3)(0, 0, 0)
    nan12 = (C.c_float * 12)(*([float('nan')] * 12))
    assert lib.d3r_cloud_transform(0, one, M, one, None, None, None, None) == -1
    assert lib.d3r_cloud_transform(4, one, nan12, one, None, None, None, None) == -1
    assert lib.d3r_cloud_transform(4, one, None, one, None, None, None, None) == -1
    assert lib.d3r_cloud_transform(4, one, M, one, one, R, None, None) == -1          # normals on one side only
    assert lib.d3r_cloud_transform(4, one, M, one, one, None, one, None) == -1        # normals without their rotation
    sums = lambda **kw: lib.d3r_cloud_icp_sums(*[dict(dict(n=4, moved=one, mn=None, n_ref=4, ref=one, rn=one, d2=one, idx=one, metric=1, gate=1.0,      # noqa: E731
                                                            cos=0.0, centre=c, count=one, sums=one, used=None, work=one, stream=None), **kw)[k]
                                                 for k in ('n', 'moved', 'mn', 'n_ref', 'ref', 'rn', 'd2', 'idx', 'metric', 'gate', 'cos', 'centre', 'count',
                                                           'sums', 'used', 'work', 'stream')])
    for kw in (dict(n=0), dict(n_ref=0), dict(metric=2), dict(gate=0.0), dict(gate=float('nan')), dict(gate=1e30), dict(rn=None),
               dict(metric=0, rn=None, mn=one), dict(mn=one, cos=float('nan')), dict(centre=None), dict(work=None), dict(idx=None)):
        assert sums(**kw) == -1, kw


def test_command_line_arguments():
    from dust3r_amd.evaluation import parse_args
    a = parse_args(['p.ply', 'g.ply', '--max-dist', '0.5'])
    assert not a.register and a.init is None and not a.rigid and a.metric == 'plane' and a.register_dist is None and a.thresholds is None
    a = parse_args(['p.ply', 'g.ply', '--max-dist', '0.5', '--register', '--init', 'S.txt', '--rigid', '--metric', 'point', '--register-dist', '2', '1', '0.5'])
    assert a.register and a.init == 'S.txt' and a.rigid and a.metric == 'point' and a.register_dist == [2.0, 1.0, 0.5] and a.max_dist == 0.5
    for bad in (['--rigid'], ['--init', 'S.txt'], ['--register-dist', '1'], ['--metric', 'point'], ['--register', '--metric', 'line']):
        with pytest.raises(SystemExit):
            parse_args(['p.ply', 'g.ply', '--max-dist', '0.5'] + bad)
