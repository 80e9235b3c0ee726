"""Cloud-to-cloud metrics on the GPU: the kernels of csrc/cloud_nn.hip against the numpy restatements of tests/test_cloud_metrics_cpu.py.
Nearest neighbours are compared exactly (np.array_equal on d2 and idx): the definition is an fp32 brute force over all pairs, the kernel
evaluates the same fp32 expression on a subset that always holds every point within r, so there is nothing to tolerate. The clouds are a few
thousand points: brute force in numpy stays below 25 M pairs a case."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from test_cloud_metrics_cpu import brute_force, lattice_case, restated_grid_nearest
from test_fuse_cpu import check_cloud, restated_fuse

pytestmark = pytest.mark.gpu


def single_pass(Q, R, r, cell, gpu, evals=False):
    """one (build, query) pair of the C ABI at a cell size of the caller's choice"""
    from dust3r_amd._lib import check, current_stream, lib, ptr
    from dust3r_amd.cloud_metrics import _bounds
    from dust3r_amd.viz import fuse_key_bits
    Qd, Rd = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).to(gpu), torch.from_numpy(np.ascontiguousarray(R, np.float32)).to(gpu)
    nq, nr = len(Qd), len(Rd)
    with torch.cuda.device(gpu):
        lo, hi, n_valid = _bounds(Rd, gpu)
        assert n_valid == int(np.isfinite(R).all(axis=1).sum())
        bits = fuse_key_bits(lo, hi, cell)
        lo_c, bits_c = (C.c_float * 3)(*lo.tolist()), (C.c_int * 3)(*bits)
        work = torch.empty(int(lib.d3r_cloud_grid_workspace_bytes(nr, nq)), dtype=torch.uint8, device=gpu)
        d2 = torch.full((nq,), -7.0, device=gpu)                       # poison: every row must be written
        idx = torch.full((nq,), -7, dtype=torch.int32, device=gpu)
        ev = torch.zeros((nq,), dtype=torch.int32, device=gpu) if evals else None
        check(lib.d3r_cloud_grid_build(nr, ptr(Rd), lo_c, float(np.float32(cell)), bits_c, ptr(work), current_stream()), 'build')
        check(lib.d3r_cloud_nearest(nr, nq, ptr(Qd), float(np.float32(r)), lo_c, float(np.float32(cell)), bits_c, 0, ptr(d2), ptr(idx), ptr(ev), ptr(work),
                                    current_stream()), 'nearest')
    out = (d2.cpu().numpy(), idx.cpu().numpy())
    return out + (ev.cpu().numpy(),) if evals else out


def assert_same(got, want, what=''):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0], want[0]), what


@pytest.mark.parametrize('n_ref', [1, 1023, 1025, 4097])
def test_sort_tile_edges(gpu, n_ref):
    """reference clouds of one point, one tile - 1, one tile + 1 and one sort tile + 1; 1531 queries (no multiple of 256)"""
    from dust3r_amd.cloud_metrics import nearest_in_cloud
    rng = np.random.default_rng(n_ref)
    R, Q = rng.random((n_ref, 3)).astype(np.float32), rng.random((1531, 3)).astype(np.float32)
    r = 0.5 if n_ref == 1 else 0.05
    want = brute_force(Q, R, r)
    assert 0 < (want[1] >= 0).sum() < len(Q)
    for cell in (r / 2, r, 2 * r):
        assert_same(single_pass(Q, R, r, cell, gpu), want, cell)
    assert_same(nearest_in_cloud(Q, R, r), want)


@pytest.mark.parametrize('factor', [0.5, 1.0, 2.0])
def test_lattice_clouds(gpu, factor):
    """spacing r: distances exactly r (accepted) and exactly 2 r (refused), ties and duplicate reference points (the lowest index), queries
    one and two spacings outside every face of the grid"""
    rng = np.random.default_rng(21)
    for r in (0.25, 1e-3):
        Q, R = lattice_case(rng, r, 0.0, side=6)
        want = brute_force(Q, R, r)
        r2 = np.float32(r) * np.float32(r)
        assert (want[0] == r2).sum() > 20 and (want[0] == 0).sum() > 20 and (want[1] < 0).sum() > 20
        got = single_pass(Q, R, r, np.float32(r) * np.float32(factor), gpu, evals=True)
        assert_same(got, want, r)
        assert np.array_equal(got[2], restated_grid_nearest(Q, R, r, np.float32(r) * np.float32(factor))[2])      # and it looked at the same cells


@pytest.mark.parametrize('offset', [1000.0, -37.3, 5e4])
def test_large_offsets(gpu, offset):
    """r = 1e-3 at offsets up to 5e4, where one ulp (3.9e-3) exceeds r: the lattice collapses onto the representable numbers"""
    rng = np.random.default_rng(22)
    Q, R = lattice_case(rng, 1e-3, offset, side=6)
    want = brute_force(Q, R, 1e-3)
    assert (want[1] >= 0).any()
    for factor in (0.5, 1.0, 2.0):
        assert_same(single_pass(Q, R, 1e-3, np.float32(1e-3) * np.float32(factor), gpu), want, factor)


def test_planar_cloud_crowded_cell_and_nonfinite_points(gpu):
    from dust3r_amd.cloud_metrics import nearest_in_cloud
    rng = np.random.default_rng(23)
    R = (rng.random((5000, 3)) * np.float32([4, 2, 0])).astype(np.float32)               # planar: one axis has a single cell
    R[:3000] = np.float32([1.03, 1.02, 0]) + (rng.random((3000, 3)) * np.float32([0.04, 0.04, 0])).astype(np.float32)      # 3000 points in one cell of 0.1
    Q = (rng.random((3001, 3)) * np.float32([5, 3, 0.3]) - np.float32([0.5, 0.5, 0.15])).astype(np.float32)
    Q[:600] = np.float32([1.0, 1.0, -0.05]) + (rng.random((600, 3)) * np.float32([0.1, 0.1, 0.1])).astype(np.float32)       # queries around the crowd
    R[3000::97, 1], R[3005::131, 0], R[3007::201, 2] = np.nan, np.inf, -np.inf
    Q[::89, 0], Q[3::113, 2] = np.inf, np.nan
    want = brute_force(Q, R, 0.1)
    assert (want[1] >= 0).sum() > 1000 and (want[1] < 0).sum() > 500
    got = single_pass(Q, R, 0.1, 0.1, gpu, evals=True)
    assert_same(got, want)
    assert got[2].max() >= 3000                                        # the crowded cell was walked point by point
    assert_same(single_pass(Q, R, 0.1, 0.05, gpu), want)
    assert_same(single_pass(Q, R, 0.1, 100.0, gpu), want)              # one cell holds the whole cloud: slow, not wrong
    assert_same(nearest_in_cloud(Q, R, 0.1), want)


def test_empty_sides(gpu):
    from dust3r_amd.cloud_metrics import cloud_metrics, nearest_in_cloud
    rng = np.random.default_rng(24)
    Q = rng.random((300, 3)).astype(np.float32)
    nothing = np.full((200, 3), np.nan, np.float32)                    # an empty reference after validity filtering
    d2, idx = nearest_in_cloud(Q, nothing, 0.5)
    assert np.isinf(d2).all() and (idx == -1).all() and d2.dtype == np.float32 and idx.dtype == np.int32
    for empty in (np.zeros((0, 3), np.float32), torch.zeros((0, 3), device=gpu)):
        d2, idx = nearest_in_cloud(Q, empty, 0.5)
        assert np.isinf(d2).all() and (idx == -1).all() and len(idx) == 300
        d2, idx = nearest_in_cloud(empty, Q, 0.5)                      # an empty query set
        assert d2.shape == (0,) and idx.shape == (0,)
    m = cloud_metrics(Q, nothing, 0.5, [0.1])
    assert math.isnan(m['accuracy']) and math.isnan(m['completeness']) and m['n_valid_gt'] == 0 and m['n_valid_pred'] == 300 and m['precision'] == [0.0]
    assert math.isnan(m['recall'][0]) and m['outliers_pred'] == 1.0


def test_ladder(gpu):
    """max_dist = 64 r_0: four passes (r_0, 4 r_0, 16 r_0, 64 r_0). The queries are drawn at every scale from the reference cloud, so each pass
    resolves some and some are never resolved; the result is the single brute force at max_dist, and a second call gives the same bytes."""
    from dust3r_amd.cloud_metrics import ladder_radii, nearest_in_cloud
    rng = np.random.default_rng(25)
    R = rng.random((4000, 3)).astype(np.float32)
    scale = np.float32(10.0) ** rng.uniform(-3.5, 0.3, size=(3000, 1)).astype(np.float32)
    Q = (R[rng.integers(0, len(R), 3000)] + scale * rng.standard_normal((3000, 3)).astype(np.float32)).astype(np.float32)
    Q[:200] += np.float32(5)                                           # far away: never resolved
    r0, max_dist = 0.004, 0.256
    radii = ladder_radii(r0, max_dist)
    assert len(radii) == 4 and radii[-1] == np.float32(max_dist)
    found = [int((brute_force(Q, R, r)[1] >= 0).sum()) for r in radii]
    assert 0 < found[0] < found[1] < found[2] < found[3] < len(Q) - 100, found
    want = brute_force(Q, R, max_dist)
    a = nearest_in_cloud(Q, R, max_dist, r0=r0)
    assert_same(a, want)
    b = nearest_in_cloud(torch.from_numpy(Q).to(gpu), torch.from_numpy(R).to(gpu), max_dist, r0=r0, to_host=False)
    assert b[0].is_cuda and b[1].is_cuda
    assert a[0].tobytes() == b[0].cpu().numpy().tobytes() and a[1].tobytes() == b[1].cpu().numpy().tobytes()
    assert_same(nearest_in_cloud(Q, R, max_dist), want)                # the default r_0 = max_dist / 16


@pytest.mark.parametrize('n', [5000, 300001])
def test_statistics(gpu, n):
    """5000 rows: one partial per workgroup of 256; 300001 rows: past 1024 workgroups, the grid-stride loop. Counts are exact; sum_d within
    (N + 1) 2^-52 relative of math.fsum over np.sqrt(float64(d2)) (one rounding per term, then a fixed-order sum of N non-negative terms);
    sum_d2 by the same bound; the median is the element of rank (n_found - 1) / 2; two runs give the same bytes."""
    from dust3r_amd.cloud_metrics import distance_stats
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3)).astype(np.float32)
    pts[::41, 1] = np.nan
    valid = np.isfinite(pts).all(axis=1)
    found = valid & (rng.random(n) < 0.8)
    d2 = np.where(found, (rng.random(n) ** 3).astype(np.float32), np.float32(np.inf)).astype(np.float32)
    idx = np.where(found, rng.integers(0, 1000, n), -1).astype(np.int32)
    tau = [0.1, 0.5, float(np.sqrt(d2[found][5])), 0.0, 2.0]
    dev = [torch.from_numpy(a).to(gpu) for a in (pts, d2, idx)]
    runs = [[t.cpu().numpy() for t in distance_stats(*dev, tau)] for _ in range(2)]
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    counts, sums, median = runs[0]
    f = d2[found]
    assert counts[0] == valid.sum() and counts[1] == found.sum()
    want = [int((f <= np.float32(t) * np.float32(t)).sum()) for t in tau]
    assert counts[2:7].tolist() == want and counts[7:].tolist() == [0, 0, 0] and 0 < want[3] + 1 <= want[0] < want[1] < want[4] == len(f)
    bound = (len(f) + 1) * 2.0 ** -52
    s_d, s_d2 = math.fsum(np.sqrt(f.astype(np.float64))), math.fsum(f.astype(np.float64))
    print(f'n = {n}: sum_d {sums[0]!r} against {s_d!r} (relative {abs(sums[0] - s_d) / s_d:.3e}, bound {bound:.3e}); sum_d2 relative {abs(sums[1] - s_d2) / s_d2:.3e}')
    assert abs(sums[0] - s_d) <= bound * s_d and abs(sums[1] - s_d2) <= bound * s_d2
    assert median[0] == np.sort(f)[(len(f) - 1) // 2]
    none = distance_stats(dev[0], dev[1], torch.full_like(dev[2], -1), tau)
    assert none[0].tolist()[:3] == [int(valid.sum()), 0, 0] and none[1].tolist() == [0.0, 0.0] and math.isnan(float(none[2][0]))
    allq = distance_stats(None, dev[1], dev[2], [])                    # no points: every row counts as valid
    assert allq[0].tolist() == [n, int(found.sum())] + [0] * 8


def test_error_returns(gpu):
    """the C entry points refuse what they cannot run, before any launch"""
    from dust3r_amd._lib import current_stream, lib, ptr
    nr, nq = 64, 40
    R, Q = torch.rand((nr, 3), device=gpu), torch.rand((nq, 3), device=gpu)
    work = torch.empty(int(lib.d3r_cloud_grid_workspace_bytes(nr, nq)) + int(lib.d3r_cloud_distance_stats_workspace_bytes(nq)), dtype=torch.uint8, device=gpu)
    d2, idx = torch.empty(nq, device=gpu), torch.empty(nq, dtype=torch.int32, device=gpu)
    counts, sums = torch.empty(10, dtype=torch.int64, device=gpu), torch.empty(2, dtype=torch.float64, device=gpu)

    def host(ctype, values):                                           # a HOST array argument, or NULL
        return None if values is None else (ctype * max(len(values), 1))(*values)

    def build(lo=(0.0, 0.0, 0.0), cell=0.25, bits=(3, 3, 3), **kw):
        a = dict(dict(n=nr, ref=ptr(R), work=ptr(work)), **kw)
        return lib.d3r_cloud_grid_build(a['n'], a['ref'], host(C.c_float, lo), cell, host(C.c_int, bits), a['work'], current_stream())

    def nearest(lo=(0.0, 0.0, 0.0), cell=0.25, bits=(3, 3, 3), r=0.25, **kw):
        a = dict(dict(nr=nr, nq=nq, q=ptr(Q), d2=ptr(d2), idx=ptr(idx), work=ptr(work)), **kw)
        return lib.d3r_cloud_nearest(a['nr'], a['nq'], a['q'], r, host(C.c_float, lo), cell, host(C.c_int, bits), 0, a['d2'], a['idx'], None, a['work'],
                                     current_stream())

    def stats(tau=(0.1, 0.2), n_tau=None, **kw):
        a = dict(dict(n=nq, d2=ptr(d2), idx=ptr(idx), counts=ptr(counts), sums=ptr(sums), work=ptr(work)), **kw)
        return lib.d3r_cloud_distance_stats(a['n'], ptr(Q), a['d2'], a['idx'], len(tau) if n_tau is None else n_tau, host(C.c_float, tau),
                                            a['counts'], a['sums'], a['work'], current_stream())
    assert build() == 0 and nearest() == 0 and stats() == 0
    bad_grid = (dict(cell=0.0), dict(cell=-1.0), dict(cell=float('nan')), dict(cell=float('inf')), dict(bits=(0, 3, 3)), dict(bits=(3, 22, 3)),
                dict(lo=(0.0, float('nan'), 0.0)), dict(lo=(float('inf'), 0.0, 0.0)), dict(lo=None), dict(bits=None), dict(work=None))
    for kw in bad_grid + (dict(n=0), dict(n=-5), dict(ref=None)):
        assert build(**kw) == -1, kw
    for kw in bad_grid + (dict(nr=0), dict(nq=0), dict(nq=-1), dict(q=None), dict(d2=None), dict(idx=None), dict(r=0.0), dict(r=-0.5), dict(r=float('nan')),
                          dict(r=float('inf')), dict(r=1e-20), dict(r=1.0e-19), dict(r=1.9e19), dict(r=3e38)):      # r r subnormal / infinite
        assert nearest(**kw) == -1, kw
    assert nearest(r=1.2e-19) == 0 and nearest(r=1.8e19) == 0 and nearest() == 0      # the ends of the range of r, then the call checked below
    for kw in (dict(n=0), dict(d2=None), dict(idx=None), dict(counts=None), dict(sums=None), dict(work=None), dict(n_tau=-1), dict(n_tau=9),
               dict(tau=(0.1, -0.1)), dict(tau=(float('nan'),)), dict(tau=(float('inf'),)), dict(tau=None, n_tau=2)):
        assert stats(**kw) == -1, kw
    torch.cuda.synchronize()
    want = brute_force(Q.cpu().numpy(), R.cpu().numpy(), 0.25)         # the good calls ran
    assert np.array_equal(idx.cpu().numpy(), want[1]) and counts[0].item() == nq and counts[1].item() == int((want[1] >= 0).sum())


def _restated_side(P, d2, idx, thresholds):
    f = d2[idx >= 0].astype(np.float64)
    return dict(n_valid=int(np.isfinite(P).all(axis=1).sum()), n_found=len(f), sum_d=math.fsum(np.sqrt(f)), sum_d2=math.fsum(f),
                median_d2=float(np.sort(f)[(len(f) - 1) // 2]) if len(f) else float('nan'),
                counts=[int((d2[idx >= 0] <= np.float32(t) * np.float32(t)).sum()) for t in thresholds])


def restated_metrics(P, G, max_dist, thresholds):
    from dust3r_amd.cloud_metrics import compose_metrics
    return compose_metrics(_restated_side(P, *brute_force(P, G, max_dist), thresholds), _restated_side(G, *brute_force(G, P, max_dist), thresholds), thresholds)


def assert_metrics(got, want, n):
    """counts, medians and thresholds equal; the sums (and what is composed of them) within the bound of test_statistics"""
    assert sorted(got) == sorted(want)
    tol = (n + 1) * 2.0 ** -51
    for k, w in want.items():
        g = got[k]
        if isinstance(w, list) or isinstance(w, int) or k.startswith('median') or k.endswith('_median'):
            assert g == w or (isinstance(w, float) and math.isnan(w) and math.isnan(g)), k
        else:
            assert (math.isnan(w) and math.isnan(g)) or abs(g - w) <= tol * abs(w), (k, g, w)


def test_cloud_metrics_against_the_composed_restatement(gpu):
    from dust3r_amd.cloud_metrics import cloud_metrics
    from dust3r_amd.viz import FusedCloud
    rng = np.random.default_rng(26)
    G = np.concatenate([rng.random((4000, 3)), rng.random((500, 3)) - 0.8]).astype(np.float32)
    P = np.concatenate([G[:2500] + np.float32(0.01) * rng.standard_normal((2500, 3)).astype(np.float32), rng.random((700, 3)).astype(np.float32) + np.float32(0.7)])
    P[::53, 2] = np.nan
    G[::71, 0] = np.inf
    thresholds = [0.005, 0.02, 0.08]
    want = restated_metrics(P, G, 0.08, thresholds)
    assert 0.1 < want['outliers_pred'] < 0.5 and 0.05 < want['outliers_gt'] < 0.9 and 0 < want['fscore'][0] < want['fscore'][2] < 1
    got = cloud_metrics(P, G, 0.08, thresholds)
    assert_metrics(got, want, len(G))
    details = {}
    dev = cloud_metrics(torch.from_numpy(P).to(gpu), torch.from_numpy(G).to(gpu), 0.08, thresholds, to_host=False, details=details)
    assert dev['pred'][0].is_cuda and dev['pred'][0][:2].tolist() == [want['n_valid_pred'], want['n_found_pred']] and dev['gt'][1].dtype == torch.float64
    assert np.array_equal(details['idx_gt'].cpu().numpy(), brute_force(G, P, 0.08)[1])
    cloud = FusedCloud(P, np.zeros((len(P), 3), np.uint8), np.ones(len(P), np.float32), np.ones(len(P), np.int32), 0.004, (P[0], P[0]))
    assert_same(cloud.distance_to(G, 0.08), brute_force(P, G, 0.08))   # r_0 = twice the cloud's... the other side has no voxel size: max_dist / 16
    other = FusedCloud(G, np.zeros((len(G), 3), np.uint8), np.ones(len(G), np.float32), np.ones(len(G), np.int32), 0.004, (G[0], G[0]))
    assert_same(cloud.distance_to(other, 0.08), brute_force(P, G, 0.08))      # r_0 = 0.008: four passes


# ---- evaluate_scene ---------------------------------------------------------------------------------------------------------------------
N_VIEWS, H, W = 4, 24, 32


@pytest.fixture(scope='module')
def scene_and_gt(gpu):
    """synthetic_scene(4 views, 24 x 32, perturb=False) loaded into an aligner: the scene IS the ground truth in a world scaled by
    gt['world_scale']; the ground-truth views are built from gt (cam2world, focal, depth)."""
    from dust3r_amd.cloud_opt import global_aligner
    from dust3r_amd.synthetic import outdoor_scene, synthetic_scene
    out, init, gt = synthetic_scene(N_VIEWS, H, W, seed=1, scene_graph='complete', symmetrize=True, noise=0.002, device=gpu, perturb=False)
    scene = global_aligner(out, device=gpu, verbose=False)
    scene.load_state_dict(init)
    scene.imgs = [outdoor_scene(H, W, seed=k).astype(np.float32) / 255 for k in range(N_VIEWS)]
    scene.min_conf_thr = float(scene._im_conf[:, :H * W].median())      # the scene's mask keeps half of the pixels
    c2w, f, depth = gt['cam2world'].numpy().astype(np.float64), float(gt['focal']), gt['depth'].numpy().astype(np.float64)
    vs, us = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    rays = np.stack(((us - W / 2) / f, (vs - H / 2) / f, np.ones_like(us)), axis=-1)
    rng = np.random.default_rng(3)
    views = []
    for k in range(N_VIEWS):
        pts = (depth[k][..., None] * rays) @ c2w[k, :3, :3].T + c2w[k, :3, 3]
        views.append(dict(pts3d=pts.astype(np.float32), valid_mask=rng.random((H, W)) < 0.9, camera_pose=c2w[k].astype(np.float32)))
    return scene, views, gt


def umeyama(x, y, dtype):
    """numpy Umeyama x -> y (n, 3) evaluated in `dtype`: the 4 x 4 [s R | t]"""
    x, y = x.astype(dtype), y.astype(dtype)
    mx, my = x.mean(axis=0), y.mean(axis=0)
    xc, yc = x - mx, y - my
    cov = (yc.T @ xc) / dtype(len(x))
    var = (xc * xc).sum() / dtype(len(x))
    U, S, Vt = np.linalg.svd(cov)
    d = np.ones(3, dtype)
    d[2] = np.sign(np.linalg.det(U @ Vt)) or 1
    Rm = (U * d) @ Vt
    s = (S * d).sum() / var
    out = np.eye(4, dtype=dtype)
    out[:3, :3], out[:3, 3] = s * Rm, my - s * Rm @ mx
    return out


def _host_views(stack, shapes):
    a = stack.detach().cpu().numpy()
    return [a[i, :h * w].reshape((h, w) + a.shape[2:]) for i, (h, w) in enumerate(shapes)]


@pytest.fixture(scope='module')
def host_scene(scene_and_gt):
    """The scene's stacks on the host, the fp64 Umeyama of its points onto the ground truth over the pixels valid on both sides, and THE
    SIMILARITY TOLERANCE both tests use: 4 x the largest deviation of the same numpy Umeyama evaluated in fp32 from its fp64 value on this
    input, measured here (about 7e-7 on entries of size 2, so about 3e-6)."""
    scene, views, gt = scene_and_gt
    shapes = [(H, W)] * N_VIEWS
    with torch.no_grad():
        pred = _host_views(scene.get_pts3d(raw=True), shapes)
        pmask = _host_views(scene.get_masks(raw=True), shapes)
        conf = _host_views(scene._im_conf, shapes)
    both = np.concatenate([(pm & v['valid_mask']).reshape(-1) for pm, v in zip(pmask, views)])
    assert 0.3 * both.size < both.sum() < 0.6 * both.size              # (half by the scene's mask, a tenth by the ground truth's)
    x, y = np.concatenate([p.reshape(-1, 3) for p in pred])[both], np.concatenate([v['pts3d'].reshape(-1, 3) for v in views])[both]
    S64 = umeyama(x, y, np.float64)
    tol = 4 * float(np.abs(umeyama(x, y, np.float32).astype(np.float64) - S64).max())
    assert 0 < tol < 1e-4
    return dict(pred=pred, pmask=pmask, conf=conf, S64=S64, tol=tol)


def assert_poses_are_the_ground_truth(m, gt, tol, what):
    """ate_rmse, |scale world_scale - 1| and the rotation errors IN RADIANS, each within the similarity tolerance. The scene's poses are fp32
    parameters (unit quaternion, signed-log translation of size 1) and the ground truth's matrices are fp32 too: their own rounding is about
    1e-7, inside the tolerance of about 3e-6, so no wider bound is needed. The angle comes from the chord (evaluation.pose_errors),
    accurate near zero."""
    worst, mean = math.radians(m['rot_err_max_deg']), math.radians(m['rot_err_mean_deg'])
    print(f"{what}: ate_rmse {m['ate_rmse']:.3e}, |scale world_scale - 1| {abs(m['scale'] * gt['world_scale'] - 1):.3e}, rotation max {worst:.3e} rad, "
          f'mean {mean:.3e} rad; tolerance {tol:.3e}')
    assert m['ate_rmse'] <= tol
    assert abs(m['scale'] * gt['world_scale'] - 1) <= tol
    assert 0 <= mean <= worst <= tol


def test_evaluate_scene_stage_by_stage(gpu, scene_and_gt, host_scene):
    """Every stage of return_details against its restatement, given the stage before it.
    The similarity: numpy fp64 Umeyama on the same fp32 inputs; tolerance = 4 x the largest deviation of the SAME numpy Umeyama evaluated in
    fp32 from its fp64 value on this input, measured in the fixture (printed; about 1e-6 on entries of size 2) -- the kernel's moments are fp32
    products summed in fp64, which must not be worse than an all-fp32 evaluation, and the factor 4 covers the different summation order.
    The recovered scale times world_scale is 1, and the poses moved by the similarity are the ground truth's (ate_rmse, rotation in radians),
    all within that tolerance."""
    from dust3r_amd.evaluation import evaluate_scene
    scene, views, gt = scene_and_gt
    shapes = [(H, W)] * N_VIEWS
    metrics, det = evaluate_scene(scene, views, return_details=True)
    pred, pmask, conf, S64, tol = (host_scene[k] for k in ('pred', 'pmask', 'conf', 'S64', 'tol'))
    print(f'similarity: fp32 numpy Umeyama deviates {tol / 4:.3e} from fp64; tolerance {tol:.3e}; kernel {np.abs(det["similarity"] - S64).max():.3e}')
    assert np.abs(det['similarity'] - S64).max() <= tol
    assert abs(det['scale'] * gt['world_scale'] - 1) <= tol and metrics['scale'] == det['scale']
    # the aligned stack: S applied in fp32
    A = det['similarity']
    moved = _host_views(det['pred_pts'], shapes)
    for m, p in zip(moved, pred):
        want = p.astype(np.float64) @ A[:3, :3].T + A[:3, 3]
        assert np.abs(m - want).max() <= 2.0 ** -20 * (np.abs(want).max() + 1)
    # the clouds: the fusion of exactly these stacks
    v = det['voxel_size']
    gmask = [vw['valid_mask'] for vw in views]
    check_cloud(det['pred_cloud'], restated_fuse(scene.imgs, moved, pmask, conf, v))
    check_cloud(det['gt_cloud'], restated_fuse(scene.imgs, [vw['pts3d'] for vw in views], gmask, None, v))
    assert np.array_equal(det['gt_mask'].cpu().numpy()[:, :H * W].reshape(N_VIEWS, H, W), np.stack(gmask))
    # the distances: brute force between exactly these clouds
    P, G = det['pred_cloud'].positions.cpu().numpy(), det['gt_cloud'].positions.cpu().numpy()
    assert det['max_dist'] == 16 * v and det['thresholds'] == [v, 2 * v, 4 * v] and len(P) > 1000 and len(G) > 1000
    for side, (a, b) in (('pred', (P, G)), ('gt', (G, P))):
        want = brute_force(a, b, det['max_dist'])
        assert np.array_equal(det[f'd2_{side}'].cpu().numpy(), want[0]) and np.array_equal(det[f'idx_{side}'].cpu().numpy(), want[1]), side
    # the metrics: composed from these distances
    want = restated_metrics(P, G, det['max_dist'], det['thresholds'])
    got = {k: metrics[k] for k in want}
    assert_metrics(got, want, max(len(P), len(G)))
    assert metrics['accuracy'] < v and metrics['completeness'] < v and metrics['fscore'][2] > 0.9        # the scene is the ground truth
    # the poses, moved by S, are the ground truth's
    assert_poses_are_the_ground_truth(metrics, gt, tol, "align='points'")
    assert set(evaluate_scene(scene, views)) == set(metrics)


def test_evaluate_scene_unaligned_shift_and_poses(gpu, scene_and_gt, host_scene):
    """align=None against the scene's own points shifted by three voxels along x: accuracy is what the restatement gives, and that lies
    between 2 and 4 voxels. The voxel is a quarter of the scene's default: at the default the four 24 x 32 views' surfaces lie 2 to 5 voxels
    from each other and a shifted point finds another view's surface after 1.2 voxels (measured on the host); at a quarter the nearest point
    is on the point's own, shifted surface (2.6). align='poses' registers by the cameras alone: ate_rmse, the rotation errors in radians and
    |scale world_scale - 1| are zero within the similarity's tolerance (the fixture's, measured on this scene)."""
    from dust3r_amd.evaluation import evaluate_scene
    from dust3r_amd.viz import default_voxel_size
    scene, views, gt = scene_and_gt
    pred, pmask, conf = (host_scene[k] for k in ('pred', 'pmask', 'conf'))
    with torch.no_grad():
        v = default_voxel_size(scene.get_depthmaps(raw=True), [H * W] * N_VIEWS, scene.get_focals()) / 4
    shift = np.float32([3 * v, 0, 0])
    shifted = [dict(pts3d=p + shift, valid_mask=np.ones((H, W), bool)) for p in pred]
    P = restated_fuse(scene.imgs, pred, pmask, conf, v)['positions']
    G = restated_fuse(scene.imgs, [s['pts3d'] for s in shifted], [s['valid_mask'] for s in shifted], None, v)['positions']
    want = restated_metrics(P, G, 16 * v, [v, 2 * v, 4 * v])
    print(f'restated accuracy under a shift of 3 voxels: {want["accuracy"] / v:.3f} voxels')
    assert 2 * v < want['accuracy'] < 4 * v
    got = evaluate_scene(scene, shifted, align=None, voxel_size=v)
    assert got['scale'] == 1.0 and 'ate_rmse' not in got and got['n_found_pred'] == want['n_found_pred']
    assert abs(got['accuracy'] - want['accuracy']) <= (len(P) + 1) * 2.0 ** -51 * want['accuracy']
    m = evaluate_scene(scene, views, align='poses')
    assert_poses_are_the_ground_truth(m, gt, host_scene['tol'], "align='poses'")
    with pytest.raises(ValueError, match="align='poses' needs camera_pose"):
        evaluate_scene(scene, shifted, align='poses')
    with pytest.raises(ValueError, match="align is 'points', 'poses' or None"):
        evaluate_scene(scene, views, align='icp')
    with pytest.raises(ValueError, match='ground-truth views'):
        evaluate_scene(scene, views[:2])


def test_resource_report_has_no_scratch():
    """read only: the report is what the build left next to the object; nothing is built or touched here"""
    from dust3r_amd import _lib
    path = os.path.join(os.path.dirname(_lib.LIB_PATH), 'cloud_nn.resources.txt')
    if not os.path.exists(path):
        pytest.skip('no cloud_nn.resources.txt: the library was not built by dust3r_amd/build.py')
    report = open(path).read()
    kernels = re.findall(r'Function Name: (\S+)', report)
    new = [k for k in kernels if 'cloud_' in k]
    assert len(new) == 5 and len(kernels) == 12 and sum('cloud_sums_final_kernel' in k for k in new) == 1 and all('cloud_' in k or 'fuse_' in k for k in kernels)
    assert re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', report) == ['0'] * len(kernels)
